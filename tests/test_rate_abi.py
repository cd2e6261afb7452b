"""CPU-side checks of the batch byte budget and the constant bitrate (m1v_encode_batch_budget_device, m1v_encode_cbr_device,
include/mpeg1_hip.h): the entry points are declared, exported and bound, a null encoder is an argument error without a device,
the pick kernel is in the gfx950 code object with the shape the design needs, and the two rules (the reference models that
tests/test_gpu_rate.py checks the device against) keep their promises on random tables."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from code_object import _gfx950_disassembly
from rate_rules import batch_rule, batch_rule_prefix_test, cbr_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {"m1v_encode_batch_budget_device": 14, "m1v_encode_cbr_device": 17}


# ---- the rules, as include/mpeg1_hip.h states them ------------------------------------------------------------------------


def _random_table(rng, K, n, monotone):
    base = rng.integers(60, 4000, n)
    if monotone:
        steps = rng.integers(0, 900, (K, n)).cumsum(axis=0)
        return (base + steps).tolist()
    return (base + rng.integers(-300, 900, (K, n)).cumsum(axis=0)).clip(48).tolist()


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_declared_exported_and_bound():
    from ec504_imageencoder_amd import _ffi
    text = open(os.path.join(ROOT, "include", "mpeg1_hip.h")).read()
    L = _ffi.lib()
    for name, nargs in ARGS.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in _ffi.MPEG1_HIP_SYMBOLS and hasattr(L, name), name
        fn = getattr(L, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs, name


def test_null_encoder_is_an_argument_error():
    from ec504_imageencoder_amd import _ffi
    L = _ffi.lib()
    q = (C.c_uint8 * 2)(4, 8)
    assert L.m1v_encode_batch_budget_device(None, None, 0, 0, q, 2, 1000, None, None, 0, None, None, None, None) == _ffi.E_ARG
    assert "null" in _ffi.last_error()
    assert L.m1v_encode_cbr_device(None, None, 0, 0, q, 2, 100, 1000, None, None, None, None, 0, None, None, None, None) == _ffi.E_ARG
    assert "null" in _ffi.last_error()


def _pick_kernels():
    asm, notes = _gfx950_disassembly()
    bodies = {n: b for n, b in re.findall(r"<(_ZN\S*)>:\n(.*?)\n\n", asm, re.S) if "k_rate_pick" in n}
    recs = re.findall(r"\.name:\s*(\S*k_rate_pick\S*).*?\.private_segment_fixed_size:\s*(\d+)", notes, re.S)
    return bodies, recs


def test_pick_kernel_shape():
    """Both forms exist; neither uses scratch, and neither needs an atomic: one workgroup does all."""
    bodies, recs = _pick_kernels()
    assert len(bodies) == 2 and len(recs) == 2, (sorted(bodies), recs)
    for name, body in bodies.items():
        ops = [l.split("//")[0].split()[0] for l in body.splitlines() if l.strip() and not l.strip().startswith(("/", ";"))
               and len(l.split("//")[0].split()) > 0]
        assert not any(o.startswith("scratch_") or "atomic" in o for o in ops), name
    for name, scratch in recs:
        assert int(scratch) == 0, (name, scratch)


@pytest.mark.parametrize("forbidden", ["k_encode_dense", "k_encode_strips", "k_encode_tiles", "k_assemble"])
def test_pick_kernel_keeps_out_of_the_counted_names(forbidden):
    bodies, _ = _pick_kernels()
    assert bodies and not any(forbidden in n for n in bodies)


# ---- the rules ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("monotone", [True, False])
def test_batch_rule_promises(monotone):
    rng = np.random.default_rng(7 + monotone)
    for trial in range(300):
        K, n = int(rng.integers(1, 9)), int(rng.integers(1, 40))
        s = _random_table(rng, K, n, monotone)
        T = [sum(row) for row in s]
        for B in (int(rng.integers(0, 2 * max(T))), T[int(rng.integers(0, K))], T[0] - 1, max(T)):
            pick, over = batch_rule(s, B)
            total = sum(s[pick[f]][f] for f in range(n))
            assert over == (min(T) > B) if not monotone else over == (T[0] > B)
            if over:
                assert pick == [0] * n
                continue
            assert total <= B, (trial, B)
            assert max(pick) - min(pick) <= 1
            lo = min(pick)
            assert T[lo] <= B and all(T[k] > B for k in range(lo + 1, K)), (trial, B)
            assert batch_rule_prefix_test(s, B) == (pick, over), (trial, B)


def test_batch_rule_over_flag_follows_the_first_candidate():
    """Not monotone: T[0] may exceed B while a later candidate's total fits; the rule takes the largest fitting k, and the flag
    says that no uniform total fits."""
    s = [[500, 500], [300, 300], [900, 900]]
    assert batch_rule(s, 700) == ([1, 1], False)
    assert batch_rule(s, 600) == ([1, 1], False)
    assert batch_rule(s, 599) == ([0, 0], True)


def test_batch_rule_ties_by_frame_index():
    s = [[100] * 6, [110, 105, 110, 110, 90, 105]]
    # T[0] = 600; d = 10, 5, 10, 10, -10, 5; the free upgrade gives 10 back
    assert batch_rule(s, 600) == ([0, 1, 0, 0, 1, 1], False)      # room 10: d = 5 (frame 1), 5 (frame 5)
    assert batch_rule(s, 619) == ([1, 1, 0, 0, 1, 1], False)      # room 29: + frame 0 (10), frame 2 (10) does not fit
    assert batch_rule(s, 620) == ([1, 1, 1, 0, 1, 1], False)
    for B in range(590, 640):
        assert batch_rule(s, B) == batch_rule_prefix_test(s, B), B


@pytest.mark.parametrize("monotone", [True, False])
def test_cbr_rule_chains_at_any_split(monotone):
    rng = np.random.default_rng(11 + monotone)
    for trial in range(200):
        K, n = int(rng.integers(1, 9)), int(rng.integers(1, 30))
        s = _random_table(rng, K, n, monotone)
        r = int(rng.integers(1, 3000))
        C_ = r + int(rng.integers(0, 8000))
        L0 = int(rng.integers(-5000, 2 * C_))
        whole = cbr_rule(s, r, C_, L0)
        for cut in range(n + 1):
            a = cbr_rule([row[:cut] for row in s], r, C_, L0) if cut else ([], [], min(L0, C_))
            b = cbr_rule([row[cut:] for row in s], r, C_, a[2]) if cut < n else ([], [], min(a[2], C_))
            assert a[0] + b[0] == whole[0] and a[1] + [f + cut for f in b[1]] == whole[1] and b[2] == whole[2], (trial, cut)
        # what the rule promises per frame: the largest fitting candidate, the level's bounds
        L = min(L0, C_)
        for f, k in enumerate(whole[0]):
            fits = [j for j in range(K) if s[j][f] <= L]
            assert k == (fits[-1] if fits else 0) and (f in whole[1]) == (not fits)
            L = min(C_, L - s[k][f] + r)
            assert L <= C_
        assert L == whole[2]


def test_cbr_rule_debt_is_repaid():
    s = [[600, 50, 100, 100], [900, 80, 200, 150]]
    # the start is clipped to 300; frame 0 fits nothing and leaves a debt (300 - 600 + 200 = -100), frame 1 fits nothing at a
    # negative level, frame 2 nothing at 50, frame 3 takes candidate 1 at 150 exactly; the refill after it is clipped
    assert cbr_rule(s, 200, 300, 1000) == ([0, 0, 0, 1], [0, 1, 2], 200)
    assert cbr_rule(s, 200, 300, -10 ** 6)[2] == -10 ** 6 - 600 - 50 - 100 - 100 + 4 * 200
