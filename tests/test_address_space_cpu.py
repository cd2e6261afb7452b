"""tests/address_space.py on the host (no GPU): that every case is where its name says, that the setters' own arithmetic accepts
each edge and refuses the next value up, that no 32-bit slip of a kernel could leave the pool, and that each slip the model
knows would change a record — so that tests/test_gpu_address_space.py can fail."""
import numpy as np
import pytest

import address_space as A

CASES = A.cases()
IDS = [A.case_id(c) for c in CASES]
T31, T32 = A.T31, A.T32


def test_the_case_list():
    """Every layout kind, every edge it takes, the second geometry and both table modes; no id twice."""
    assert len(set(IDS)) == len(IDS) == 227
    kinds = {c.kind for c in CASES}
    assert len(kinds) == 23 and kinds == set(A.KIND)
    for k in A.kinds():
        mine = [c for c in CASES if c.kind == k.name]
        assert {c.edge for c in mine if not c.table} == set(A.edges(k))
        assert any(c.geometry == "b" for c in mine)
        assert {c.table for c in mine} == {""} | set(A.tables(k))
        assert all(c.edge in A.IN_FRAME for c in mine if c.table)
    assert {c.table for c in CASES if c.kind.startswith(("fplanes", "fpixels"))} == {""}   # (no table serves a float layout)


def test_the_pool_holds_every_slip():
    """From the pool's size alone: F - 2^31 and F + S_MAX + 2^32 lie MARGIN inside it, and the fills differ in every byte."""
    assert A.FRAME0 - T31 >= A.MARGIN and A.FRAME0 + A.S_MAX + T32 + A.MARGIN <= A.POOL_BYTES < 10.01 * 2 ** 30
    assert A.FRAME0 % 256 == 0 and A.POOL_BYTES % 4096 == 0
    a, b = A.fill_pattern("a"), A.fill_pattern("b")
    assert np.all(a != b) and len(np.unique(a)) > 100
    assert T31 % A.PERIOD and T32 % A.PERIOD        # fill 2^31 and 2^32 apart is not the same fill


def test_the_second_geometry_is_geometry_space_s():
    import geometry_space as gs
    t = gs.batch_member()
    assert (t.W, t.H) == A.GEOMETRIES["b"] and gs.shape(t.W, t.H)["mrows_here"] == 1 and gs.shape(t.W, t.H)["tile_rows"] == 2
    assert gs.shape(*A.GEOMETRIES["a"])["n_mbrows"] == 2


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_setter_arithmetic(case):
    """The setter's rule accepts the case's layout; at an edge named *_top the next value up (by the kind's alignment) is refused."""
    kind, (W, H) = A.KIND[case.kind], A.GEOMETRIES[case.geometry]
    lay, bumps = A.layout(case)
    u = A.unit(kind)
    assert A.accepts(kind, lay, W, H)
    assert all(v % u == 0 for k, v in lay.items() if k.endswith(("pitch", "stride")))
    if kind.name == "samples-p010":
        assert all(lay[k] % 2 == 1 for k in ("y_offset", "cb_offset", "cr_offset"))      # the coded byte is a word's high byte
    assert bool(bumps) == (case.edge in ("pitch_top", "offset_top", "both"))
    for group in bumps:
        up = dict(lay)
        for field in group:
            up[field] += u
        assert not A.accepts(kind, up, W, H), group
        assert A.extent(kind, up, W, H) >= T32      # ... and for this reason


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_census(case):
    kind, (W, H) = A.KIND[case.kind], A.GEOMETRIES[case.geometry]
    lay, _ = A.layout(case)
    c = A.census(case)
    assert c["below"] and c["above"]            # a 16-byte unit wholly below offset 2^31 from F, and one wholly at or above it
    assert c["slips_inside"], (c["lowest"], c["highest"])
    # the last addressed byte is E - 1 (in front of it only the 4th byte or sample of the last pixel, which is skipped)
    skipped = {"surface": lambda: kind.a - 3, "float_pixels": lambda: (kind.b - 3) * A.sample_bytes(kind)}.get(kind.family, lambda: 0)()
    assert c["last_byte"] == c["extent"] - 1 - skipped and c["extent"] == A.extent(kind, lay, W, H) < T32 <= lay["frame_stride"]
    assert c["frame1"] >= T32                   # frame 1's first byte, from F
    E4 = (c["extent"] + 3) & ~3
    if case.edge in ("pitch_top", "offset_top", "both"):    # (E is at the setter's maximum: test_setter_arithmetic)
        assert c["extent"] >= T32 - 256
    if case.edge == "offset_top":
        assert E4 in (T32, T32 - 4)
        last = [o for o in A.components(case) if o.off == max(x.off for x in A.components(case))][0]
        assert last.off >= T31                  # the whole plane lies in [2^31, 2^32)
    if case.edge == "cross_31":
        if kind.family in A.YCC:
            assert c["straddles"]["Y"] and (kind.name == "samples-p010" or kind.family == "planes" or (c["straddles"]["Cb"] and c["straddles"]["Cr"]))
        else:
            assert any(c["straddles"].values())
    if case.edge == "cross_31c":
        assert c["straddles"]["Cb"] or c["straddles"]["Cr"]
    in_frame_top = max(int(A.offsets(o).max()) for o in A.components(case))
    assert (in_frame_top >= T31) == (case.edge in A.IN_FRAME + ("both",))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_discrimination(orc, case):
    """The exact rule gives the content back byte for byte; every slip that applies changes a record under both fills."""
    frames = A.content(case)
    want = A.records(orc, case, frames, A.Q_HALF)
    assert None not in want and want[0][44:] != want[1][44:] and want[0][:44] != want[1][:44]
    rules = [r for r in A.RULES if A.applies(case, r)]
    assert rules, "a case no rule can break"
    for fill in A.FILLS:
        model = A.Sparse(case, fill)
        got = A.gather(case, model)
        assert all(np.array_equal(g, f) for g, f in zip(got, frames)) if isinstance(frames, tuple) else np.array_equal(got, frames)
        for rule in rules:
            assert A.records(orc, case, A.gather(case, model, rule), A.Q_HALF) != want, (fill, rule)


def test_every_rule_is_exercised_by_every_kind():
    for k in A.kinds():
        mine = [c for c in CASES if c.kind == k.name]
        assert all(any(A.applies(c, r) for c in mine) for r in A.RULES), k.name
        assert all(any(A.applies(c, r) for c in mine if c.table == t) for t in A.tables(k) for r in ("sext", "mod31")), k.name
