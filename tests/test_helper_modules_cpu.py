"""How the suite's own modules may depend on one another, read off their syntax trees (no module of the suite is imported):
what two test modules share lives in a helper module (any tests/*.py that is neither a test module nor conftest.py), so
* no module imports a test module, at module level or inside a function: a test file can be collected and renamed on its own;
* a helper module holds nothing that pytest would collect or inject — no test_* function, no Test* class, no fixture — and no
  import *, so every name a test uses can be found where it is imported from."""
import ast
import functools
import gc
import glob
import os

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=1)
def _modules():
    """{file name: syntax tree} of tests/*.py, parsed once.  (The collector is paused meanwhile: it would walk the growing
    trees again and again, which triples the time.)"""
    out = {}
    paused = gc.isenabled()
    gc.disable()
    try:
        for path in sorted(glob.glob(os.path.join(HERE, "*.py"))):
            with open(path, encoding="utf-8") as f:
                out[os.path.basename(path)] = ast.parse(f.read(), path)
    finally:
        if paused:
            gc.enable()
    return out


def _imports(tree):
    """(line, module name, names) of every import statement of a module, wherever it stands."""
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            for a in node.names:
                yield node.lineno, a.name, ()
        elif isinstance(node, ast.ImportFrom):
            yield node.lineno, node.module or "", tuple(a.name for a in node.names)


def _is_test_module(name):
    return name.split(".")[-1].startswith("test_")


def test_no_module_imports_a_test_module():
    modules = _modules()
    assert len(modules) > 90 and "conftest.py" in modules, sorted(modules)
    found = []
    for file, tree in modules.items():
        for line, module, names in _imports(tree):
            if _is_test_module(module) or (module in ("", "tests") and any(_is_test_module(n) for n in names)):
                found.append(f"tests/{file}:{line}: imports {module or names}")
    assert not found, "\n" + "\n".join(found)


def test_helper_modules_hold_no_tests_no_fixtures_and_no_import_star():
    helpers = {f: t for f, t in _modules().items() if not f.startswith("test_") and f != "conftest.py"}
    assert len(helpers) > 20, sorted(helpers)
    found = []
    for file, tree in helpers.items():
        for node in ast.walk(tree):
            at = f"tests/{file}:{getattr(node, 'lineno', 0)}"
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                if node.name.startswith("test_") or node.name.startswith("Test"):
                    found.append(f"{at}: defines {node.name}")
                for d in node.decorator_list:
                    if "fixture" in ast.dump(d):
                        found.append(f"{at}: {node.name} is a fixture")
            elif isinstance(node, (ast.Assign, ast.AnnAssign, ast.AugAssign)) and node in tree.body:
                targets = node.targets if isinstance(node, ast.Assign) else [node.target]
                for t in targets:
                    for n in ast.walk(t):
                        if isinstance(n, ast.Name) and n.id.startswith(("test_", "Test")):
                            found.append(f"{at}: binds {n.id}")
            elif isinstance(node, ast.ImportFrom):
                for a in node.names:
                    if a.name == "*":
                        found.append(f"{at}: from {node.module} import *")
                    elif (a.asname or a.name).startswith(("test_", "Test")):
                        found.append(f"{at}: binds {a.asname or a.name}")
    assert not found, "\n" + "\n".join(found)
