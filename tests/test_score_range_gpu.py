"""GPU: every fill, batch and search path just inside and just outside the score range its arithmetic is chosen for (the table of
tests/score_range_cases.py; tests/test_score_range_host.py shows on a CPU that the oracle is exact there, that the expected routes
are the planners' and that the cases sit on their edges).  Every output a mode produces is compared bit for bit with the oracle, then
the route is asserted, so that no case passes on a path it was not meant for."""
import numpy as np
import pytest

import score_range_cases as T
from test_band_gpu import _bands

pytestmark = pytest.mark.gpu

FILLS = T.fill_cases()


def _by_group(group, **kw):
    cases = [c for c in FILLS if c.group == group and all(getattr(c, k) == v for k, v in kw.items())]
    return pytest.mark.parametrize("case", cases, ids=[c.name for c in cases])


def _dtypes(fmt):
    import torch
    return {"h32p32": (torch.int32, torch.int32), "h32p8": (torch.int32, torch.int8), "h64p32": (torch.int64, torch.int32), "none": (None, None)}[fmt]


def _fill(engine, case, a, b, out=None):
    """one fill under the case's options; returns (Fill, route)"""
    hd, pd = _dtypes(case.fmt)
    for k, v in case.options.items():
        engine.set_option(k, v)
    try:
        if out is None:
            out = engine.fill(a, b, case.scores, h_dtype=hd, p_dtype=pd, want_h=hd is not None, want_p=pd is not None)
        else:
            engine.fill_into(out, *out._seqs, case.scores)
            engine.synchronize()
        route = {"perm": engine.get_option("last_perm"), "strips2": engine.get_option("last_strips2")}
    finally:
        for k in case.options:
            engine.set_option(k, 0)
    return out, route


def _assert_route(case, route):
    assert route["perm"] == int(case.perm), f"{case.name}: last_perm {route['perm']}"
    assert (route["strips2"] > 0) == case.two_cols, f"{case.name}: last_strips2 {route['strips2']}"


def _same(case, what, got, want, H):
    """got == want, or the first wrong cell, its strip and its G-space value H - gap (row + col) + 2^16"""
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    r, c = (int(x) for x in bad[0])
    w2 = case.w2 or T.S2_W
    strip2 = 0 if c <= T.S2_W else (c - T.S2_W - 1) // w2 + 1
    g = int(H[r, c]) - case.scores[2] * (r + c) + T.kGBias
    raise AssertionError(f"{case.name}: {what} differs in {len(bad)} cells, first at row {r} col {c} (strip {(c - 1) // 63} of 63 columns, {strip2} of the "
                         f"two-column kernel), G = {g} = 2^24 - {T.kTagBit - g}; rows {bad[:, 0].min()}..{bad[:, 0].max()}, cols {bad[:, 1].min()}.."
                         f"{bad[:, 1].max()}; got {got[r, max(0, c - 2):c + 3].tolist()} want {want[r, max(0, c - 2):c + 3].tolist()}")


def _check_fill(engine, oracle, case, out, ref):
    H, P, mp = ref
    if out.H is not None:
        _same(case, "H", out.H.cpu().numpy(), H, H)   # (an int64 H against the int32 oracle: compared by value)
    if out.P is not None:
        _same(case, "P", out.P.cpu().numpy().astype(np.int32), P, H)
    r = out.result()
    assert (r["max_pos"], r["max_score"]) == (mp, int(H.flat[mp])), f"{case.name}: arg-max {r} vs {mp}, {int(H.flat[mp])}"
    if out.H is not None and out.P is not None:
        path = engine.traceback(out, mp)
        assert np.array_equal(path, oracle.backtrack(P.copy(), mp)), f"{case.name}: traceback path"


@_by_group("A")
def test_signed_byte_corners_of_the_perm_producer(engine, oracle, case):
    a, b = case.pair()
    out, route = _fill(engine, case, a, b)
    _check_fill(engine, oracle, case, out, oracle.fill(a, b, case.scores))
    _assert_route(case, route)


def _three_runs(engine, case, a, b, check):
    """twice in a row, and once after a small fill with the default scoring (another launch tag: a stale workspace must not be accepted)"""
    out, route = _fill(engine, case, a, b)
    _assert_route(case, route)
    check(out)
    first = [x.clone() if x is not None else None for x in (out.H, out.P)]
    res = out.result()
    for small in (False, True):
        if small:
            sa, sb = T.make_pair("random", 700, 300, 5)
            assert engine.fill(sa, sb).result()["max_score"] > 0
        for x in (out.H, out.P):
            if x is not None:
                x.fill_(-7)
        again, route = _fill(engine, case, a, b, out=out)
        _assert_route(case, route)
        assert again.result() == res, f"{case.name}: result of run {2 + small}"
        for what, x, y in (("H", again.H, first[0]), ("P", again.P, first[1])):
            if x is not None and not bool((x == y).all().item()):
                check(again)   # (names the first wrong cell)
                raise AssertionError(f"{case.name}: {what} of run {2 + small} differs from the first run")


@_by_group("B", streamed=False)
def test_tag_boundary(engine, oracle, case):
    a, b = case.pair()
    ref = oracle.fill(a, b, case.scores)
    if not case.inside:
        out, route = _fill(engine, case, a, b)
        _check_fill(engine, oracle, case, out, ref)
        return _assert_route(case, route)

    def fill_again_ready(out):
        if not hasattr(out, "_seqs"):
            out._seqs = (engine.to_device(a)[0], engine.to_device(b)[0])
        _check_fill(engine, oracle, case, out, ref)
        if out.P is not None and out.H is not None:   # the traceback negated the path: fill again before the runs are compared
            _assert_route(case, _fill(engine, case, a, b, out=out)[1])
    _three_runs(engine, case, a, b, fill_again_ready)


@_by_group("B", streamed=True)
def test_tag_boundary_streamed(engine, oracle, case):
    """4.2e8 cells: row checksums of H and P, the bottom row and the arg-max against the streaming oracle"""
    a, b = case.pair()
    st = oracle.fill_streaming(a, b, case.scores)

    def check(out):
        out._seqs = (engine.to_device(a)[0], engine.to_device(b)[0])
        r = out.result()
        assert (r["max_pos"], r["max_score"]) == (st["max_pos"], st["max_score"])
        assert np.array_equal(out.H[-1].cpu().numpy(), st["bottom"]), "bottom row"
        for what, X, want in (("H", out.H, st["csH"]), ("P", out.P, st["csP"])):
            got = engine.row_checksums(X)
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, f"{case.name}: {what} row checksums differ in {len(bad)} rows, first {bad[0]}"
    _three_runs(engine, case, a, b, check)


def test_tag_boundary_stacked_bands(engine, oracle, swamd):
    """three bands of a corner input as wide as the perm producer takes them: the halo rows carry the climbing diagonal"""
    cols, total, cuts, scores = T.band_case()
    _bands(engine, oracle, swamd, cols, total, cuts, scores=scores, ab=T.make_pair("corner", cols, total, 99))
    assert engine.get_option("last_perm") == 1 and engine.get_option("last_strips2") > 0


@_by_group("C", valid=True)
def test_outer_limits_of_check_dims(engine, oracle, swamd, case):
    a, b = case.pair()
    ref = oracle.fill(a, b, case.scores)
    out, route = _fill(engine, case, a, b)
    _check_fill(engine, oracle, case, out, ref)
    _assert_route(case, route)
    if case.fmt == "h32p32" and case.options["engine"] == 0:   # ... and sw_fill_host and the batch fall-back, once per input
        H, P, mp = ref
        r = swamd.fill_host(engine, a, b, case.scores)
        _same(case, "sw_fill_host H", r["H"], H, H)
        _same(case, "sw_fill_host P", r["P"], P, H)
        assert (r["max_pos"], r["max_score"]) == (mp, int(H.flat[mp]))
        A, B = np.stack([a, a, a]), np.stack([b, b[::-1], b])
        res, bH, bP = engine.batch(A, B, scores=case.scores, store=True)
        assert engine.get_option("last_batch_kernel") == T.batch_route(case.cols, case.rows, 3, case.scores, "hp")[1]   # (the fall-back for scores beyond a byte)
        res = res.cpu().numpy()
        for k in range(3):
            h, p, m = ref if k != 1 else oracle.fill(A[1], B[1], case.scores)
            _same(case, f"batch pair {k} H", bH[k].cpu().numpy(), h, h)
            _same(case, f"batch pair {k} P", bP[k].cpu().numpy(), p, h)
            assert (res[k, 0], res[k, 1]) == (m, int(h.flat[m]))


@_by_group("C", valid=False)
def test_one_step_past_check_dims_is_rejected(engine, swamd, case):
    import torch
    a, b = case.pair()
    d_a, d_b = engine.to_device(a)[0], engine.to_device(b)[0]
    out = engine.alloc(case.cols, case.rows)
    for x in (out.H, out.P, out.res):
        x.fill_(0x5a5a5a5a)
    for k, v in case.options.items():
        engine.set_option(k, v)
    try:
        with pytest.raises(swamd.SwError) as e:
            engine.fill_into(out, d_a, d_b, case.scores)
        assert e.value.code == -22
        with pytest.raises(swamd.SwError) as e:
            swamd.fill_host(engine, a, b, case.scores)
        assert e.value.code == -22
    finally:
        for k in case.options:
            engine.set_option(k, 0)
    with pytest.raises(swamd.SwError) as e:
        engine.batch(np.stack([a, a, a]), np.stack([b, b, b]), scores=case.scores)
    assert e.value.code == -22
    with pytest.raises(swamd.SwError) as e:
        engine.search(a, [b, b[:5]], case.scores)
    assert e.value.code == -22
    engine.synchronize()
    for x in (out.H, out.P, out.res):
        assert bool((x == 0x5a5a5a5a).all().item()), "a rejected call wrote"


BATCHES = T.batch_cases()


@pytest.mark.parametrize("case", BATCHES, ids=[c.name for c in BATCHES])
def test_batch_kernels(engine, oracle, case):
    import torch
    A, B = case.pairs()
    if case.mode == "hp":
        res, H, P = engine.batch(A, B, scores=case.scores, store=True)
    elif case.mode == "p8":
        res, H, P = engine.batch(A, B, scores=case.scores, store=True, p_dtype=torch.int8, store_h=False)
    else:
        res, H, P = engine.batch(A, B, scores=case.scores, store=False)
    kernel = engine.get_option("last_batch_kernel")
    res = res.cpu().numpy()
    for k in range(case.npairs):
        h, p, mp = oracle.fill(A[k], B[k], case.scores)
        if H is not None:
            _same(case, f"pair {k} H", H[k].cpu().numpy(), h, h)
        if P is not None:
            _same(case, f"pair {k} P", P[k].cpu().numpy().astype(np.int32), p, h)
        assert (res[k, 0], res[k, 1]) == (mp, int(h.flat[mp])), f"{case.name}: pair {k} arg-max {res[k].tolist()} vs {mp}, {int(h.flat[mp])}"
    assert kernel == case.kernel, f"{case.name}: last_batch_kernel {kernel}"


SEARCHES = T.search_cases()


@pytest.mark.parametrize("case", SEARCHES, ids=[c.name for c in SEARCHES])
def test_search_kernels(engine, oracle, case):
    query, packed, offs = case.data()
    scores = case.scores_for(offs)
    res = engine.search(query, (packed, offs), scores)
    assert res.shape == (len(offs) - 1, 3)
    for k in range(len(offs) - 1):
        t = packed[offs[k]:offs[k + 1]]
        o = oracle.fill_streaming(query, t, scores) if len(t) else {"max_score": 0, "max_pos": 0}
        assert (res[k, 1], res[k, 0], res[k, 2]) == (o["max_score"], o["max_pos"], 0), \
            f"{case.name}: target {k} (len {len(t)}): {tuple(res[k])} vs {o['max_score'], o['max_pos']}"
    assert engine.get_option("last_search_kernel") == case.kernel
    if case.scores and case.scores[0] > 0:
        assert res[:, 1].max() >= case.scores[0] * (case.qlen // 2 if not case.long_target else 8)   # scores climb
