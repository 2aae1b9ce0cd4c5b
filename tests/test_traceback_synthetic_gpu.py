"""GPU: the traceback kernels (csrc/sw_traceback.hip) on predecessor matrices built to break them (tests/traceback_cases.py), against a
plain reference walk on a host copy: the path index for index, path_len, and the whole matrix afterwards -- int32 / int8: every decoy
untouched and every path cell negated; 2-bit: the codes unchanged and the path bitmap equal to the reference path's, word for word.
The entry points take P as plain input, so nothing here needs a fill; the last test runs real fills whose paths hold one long LEFT or
UP run, so that the engine and the walk are also checked together.

Left out: matrices above 2^32 CELLS (an int8 matrix of 4.3 GB on the host) for host memory and time; sw_multi_traceback and the
band hop of sw_traceback_stop_device, which walk with the same kernel and are covered by the multi-GPU tests."""
import ctypes

import numpy as np
import pytest

import traceback_cases as tc

pytestmark = pytest.mark.gpu

KINDS = ["int32", "int8", "p2"]
FAMILIES = {"runs": tc.family_runs(), "alignments": tc.family_alignments(), "edges": tc.family_edges(), "shapes": tc.family_shapes(),
            "random": tc.family_random()}
ALL = [c for f in FAMILIES.values() for c in f]


def _np_dtype(kind):
    return np.int32 if kind == "int32" else np.int8


def _device_walk(engine, swamd, P, pos, kind, cap=None, extra=80):
    """Uploads P (a host matrix of codes) and walks it from pos.  cap None: through Engine.traceback / Engine.traceback_p2 (a path
    buffer of cols + rows + 2); otherwise through the C entry point with path_cap = cap and a path buffer of cap + extra entries
    pre-filled with a sentinel.  Returns (path or path buffer, path_len, matrix after the walk | (packed codes, bitmap))."""
    import torch
    rows1, m = P.shape
    if kind == "p2":
        p2, _ = tc.np_pack(P)
        dP = torch.from_numpy(p2).to("cuda")
        bits = torch.zeros((P.size + 31) // 32, dtype=torch.int32, device="cuda")
    else:
        dP = torch.from_numpy(P).to("cuda")
    if cap is None:
        if kind == "p2":
            path = engine.traceback_p2(dP, m - 1, rows1 - 1, pos, bits)
            plen = len(path)
        else:
            out = swamd.Fill(H=None, P=dP, res=torch.zeros(3, dtype=torch.int64, device="cuda"), cols=m - 1, rows=rows1 - 1)
            path = engine.traceback(out, pos)
            plen = int(out.res[2].item())
    else:
        L = swamd.lib()
        buf = torch.full((cap + extra,), tc.SENTINEL, dtype=torch.int64, device="cuda")
        res = torch.tensor([-3, -4, 77], dtype=torch.int64, device="cuda")   # (path_len < 0 on entry would mean an aborted fill)
        if kind == "p2":
            rc = L.sw_traceback_p2_device(engine._h, dP.data_ptr(), m - 1, rows1 - 1, pos, bits.data_ptr(), buf.data_ptr(), cap, res.data_ptr(), engine._stream())
        else:
            rc = L.sw_traceback_device_ex(engine._h, dP.data_ptr(), dP.element_size(), m - 1, rows1 - 1, pos, buf.data_ptr(), cap, res.data_ptr(), engine._stream())
        assert rc == 0
        engine.synchronize()
        r = res.cpu().numpy()
        assert r[0] == -3 and r[1] == -4, "the walk only writes path_len"
        path, plen = buf.cpu().numpy(), int(r[2])
    after = (dP.cpu().numpy(), bits.cpu().numpy().view(np.uint32)) if kind == "p2" else dP.cpu().numpy()
    return path, plen, after


def _assert_matrix(kind, after, P0, ref, want, msg=""):
    if kind == "p2":
        codes, bits = after
        assert np.array_equal(codes, tc.np_pack(P0)[0]), f"the walk must not modify the codes {msg}"
        assert np.array_equal(bits, tc.path_bitmap(want, P0.size)), f"path bitmap {msg}"
        assert np.array_equal(bits, tc.np_pack(ref)[1]), f"path bitmap {msg}"
    else:
        assert after.dtype == ref.dtype and np.array_equal(after, ref), f"every decoy untouched, every path cell negated {msg}"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ALL, ids=str)
def test_traceback_on_a_hand_made_matrix(engine, swamd, case, kind):
    """Families 1-5: runs around the window size, every alignment of the start cell, edge exits, small and odd shapes, random plans."""
    P0, pos = case.build(_np_dtype(kind))
    ref = P0.copy()
    want = tc.ref_walk(ref, pos)
    tc.check_property(case, ref, want)
    path, plen, after = _device_walk(engine, swamd, P0, pos, kind)
    assert plen == len(want) and len(path) == len(want)
    assert np.array_equal(path, want), f"first difference at step {int(np.argmax(path != want))}"
    _assert_matrix(kind, after, P0, ref, want)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", tc.family_caps(), ids=str)
def test_traceback_path_cap(engine, swamd, case, kind):
    """Family 6: path_cap smaller than, equal to and larger than the path.  The first min(cap, n) entries match, everything after them
    is still the sentinel, path_len is the full length and the matrix is negated along the whole path."""
    P0, pos = case.build(_np_dtype(kind))
    ref = P0.copy()
    want = tc.ref_walk(ref, pos)
    tc.check_property(case, ref, want)
    n = len(want)
    for cap in tc.cap_values(n):
        buf, plen, after = _device_walk(engine, swamd, P0, pos, kind, cap=cap, extra=n + 80 - cap)
        k = min(cap, n)
        assert plen == n, f"cap {cap}"
        assert np.array_equal(buf[:k], want[:k]), f"cap {cap}"
        assert (buf[k:] == tc.SENTINEL).all(), f"cap {cap}: wrote past min(cap, path_len)"
        _assert_matrix(kind, after, P0, ref, want, f"(cap {cap})")


def _batch_cases(npairs=37, rows1=200, m=260):
    cases = []
    for k in range(npairs):
        rng = np.random.default_rng(4000 + k)
        plan = tuple((int(rng.integers(1, 4)), int(rng.choice((1, 2, 3, 62, 63, 64, 65, 70, 130)))) for _ in range(int(rng.integers(1, 9))))
        start = (rows1 - 1, m - 1) if k % 3 == 0 else (int(rng.integers(1, rows1)), int(rng.integers(1, m)))
        cases.append(tc.Case(f"batch-{k}", rows1, m, start, plan, 4100 + k))
    return cases


@pytest.mark.parametrize("with_paths", [True, False], ids=["paths", "nopaths"])
@pytest.mark.parametrize("kind", ["int32", "int8"])
def test_batch_traceback_on_hand_made_matrices(engine, swamd, kind, with_paths):
    """sw_batch_traceback_device on 37 different matrices of one shape stacked into one buffer, max_pos per pair from a hand-written
    d_results; pair 5 enters with path_len = -1 (an aborted fill): its matrix and its path stay untouched.  path_cap is smaller than
    the longer paths, so a pair that ignored it would write into its neighbour's slots."""
    import torch
    cases = _batch_cases()
    npairs, rows1, m = len(cases), cases[0].rows1, cases[0].m
    built = [c.build(_np_dtype(kind)) for c in cases]
    P0 = np.stack([b[0] for b in built])
    ref = P0.copy()
    wants = []
    for k in range(npairs):
        wants.append(tc.ref_walk(ref[k], built[k][1]) if k != 5 else np.zeros(0, np.int64))
    ref[5] = P0[5]
    lens = [len(w) for w in wants]
    cap = 150
    assert max(lens) > cap + 64 and min(l for k, l in enumerate(lens) if k != 5) < 64 and len(tc.ref_walk(P0[5].copy(), built[5][1])) > 10
    res0 = np.zeros((npairs, 3), np.int64)
    res0[:, 0] = [b[1] for b in built]
    res0[:, 1] = 1000 + np.arange(npairs)
    res0[5, 2] = -1
    dP = torch.from_numpy(P0).to("cuda")
    dres = torch.from_numpy(res0).to("cuda")
    dpaths = torch.full((npairs, cap), tc.SENTINEL, dtype=torch.int64, device="cuda")
    rc = swamd.lib().sw_batch_traceback_device(engine._h, dP.data_ptr(), dP.element_size(), m - 1, rows1 - 1, npairs,
                                               dpaths.data_ptr() if with_paths else None, cap if with_paths else 0, dres.data_ptr(), engine._stream())
    assert rc == 0
    engine.synchronize()
    res, paths, after = dres.cpu().numpy(), dpaths.cpu().numpy(), dP.cpu().numpy()
    assert np.array_equal(res[:, :2], res0[:, :2]), "max_pos / max_score are inputs"
    assert res[5, 2] == -1
    for k in range(npairs):
        if k != 5:
            assert res[k, 2] == lens[k], f"pair {k}"
        kk = min(lens[k], cap) if with_paths else 0
        assert np.array_equal(paths[k, :kk], wants[k][:kk]) and (paths[k, kk:] == tc.SENTINEL).all(), f"pair {k} path"
        assert np.array_equal(after[k], ref[k]), f"pair {k} matrix"


# ---- family 7: the read-ahead wave (matrices above 64 MB) and offsets above 2^32 bytes ---------------------------------------------------
def _host_available_bytes():
    with open("/proc/meminfo") as f:
        for line in f:
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) * 1024
    return 0


def _need_memory(device_bytes, host_bytes):
    """The only skip in this file: decided from hipMemGetInfo / the host's available memory before anything is allocated."""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < device_bytes or _host_available_bytes() < host_bytes:
        pytest.skip(f"not enough device or host memory ({free >> 20} MiB free on the device, {device_bytes >> 20} needed; "
                    f"{_host_available_bytes() >> 20} MiB available on the host, {host_bytes >> 20} needed)")


def _big_case(rows1, m, start, background, seed):
    P = np.empty((rows1, m), np.int8)
    plan = tc.big_plan(seed)
    tc.write_path(P, start, plan, background)
    pos = start[0] * m + start[1]
    path, codes = tc.ref_walk_sparse(P, pos)
    return P, pos, path, codes


def _assert_big_path(path, codes, m):
    """Several thousand steps, LEFT and UP runs of every length of family 1 (adjacent ones merge: 300 and more), far from the
    diagonal through the start."""
    assert len(path) >= 4000 and tc.longest_run(codes, tc.LEFT) >= 300 and tc.longest_run(codes, tc.UP) >= 300
    i, j = np.divmod(path, m)
    # the read-ahead wave covers 3 lines of 128 bytes either side of the diagonal through the cursor: 96 / 384 / 1536 columns
    assert np.abs((i[0] - i) - (j[0] - j)).max() > 2000, "the path must leave the band that the read-ahead wave covers"


def test_read_ahead_wave_int8(engine, swamd):
    """int8 above 64e6 cells: the two-wave launch (a second wave reads ahead of the walk) on a path that is nowhere near the diagonal
    it prefetches; results must not depend on it."""
    import torch
    rows1, m = 8200, 8210
    assert rows1 * m > 64e6
    _need_memory(3 * rows1 * m, 4 * rows1 * m)
    P, pos, want, codes = _big_case(rows1, m, (rows1 - 1, m - 1), tc.UP, 7001)
    _assert_big_path(want, codes, m)
    dP = torch.from_numpy(P).to("cuda")
    out = swamd.Fill(H=None, P=dP, res=torch.zeros(3, dtype=torch.int64, device="cuda"), cols=m - 1, rows=rows1 - 1)
    path = engine.traceback(out, pos)
    assert int(out.res[2].item()) == len(want) and np.array_equal(path, want)
    P.reshape(-1)[want] *= -1
    assert np.array_equal(dP.cpu().numpy(), P)


def test_read_ahead_wave_p2(engine, swamd):
    """2-bit above 256e6 cells (64 MB packed), the packed bytes built on the host; the row pitch is odd, so the corner phase changes
    from window to window."""
    import torch
    rows1, m = 16100, 16101
    assert rows1 * m * 0.25 > 64e6 and m % 4 == 1
    _need_memory(rows1 * m, 5 * rows1 * m)
    P, pos, want, codes = _big_case(rows1, m, (rows1 - 2, m - 3), tc.DIAGONAL, 7002)
    _assert_big_path(want, codes, m)
    p2 = tc.pack_codes(P.reshape(-1))
    ncells = P.size
    del P
    dP2 = torch.from_numpy(p2).to("cuda")
    bits = torch.zeros((ncells + 31) // 32, dtype=torch.int32, device="cuda")
    path = engine.traceback_p2(dP2, m - 1, rows1 - 1, pos, bits)
    assert len(path) == len(want) and np.array_equal(path, want)
    assert np.array_equal(dP2.cpu().numpy(), p2), "the walk must not modify the codes"
    assert np.array_equal(bits.cpu().numpy().view(np.uint32), tc.path_bitmap(want, ncells))


def test_int32_matrix_above_4_gib(engine, swamd):
    """int32 above 2^32 bytes (the buffer size of a window is clamped to 32 bits; offsets are 64-bit): one start near the end of the
    matrix and one within the first 64 rows.  The host copy is int8, widened on the device; the matrix is compared on the device."""
    import torch
    rows1, m = 32768, 32769
    cells = rows1 * m
    assert cells * 4 > 2 ** 32
    _need_memory(7 * cells + (1 << 30), 3 * cells)
    P = np.empty((rows1, m), np.int8)
    s1 = (rows1 - 1, m - 2)
    tc.write_path(P, s1, tc.big_plan(7003), tc.LEFT)
    # the second path: within the first 64 rows (windows clamped at the top, the step walker), long LEFT runs
    s2, i, j = (50, 30000), 50, 30000
    plan2 = ((tc.LEFT, 300), (tc.DIAGONAL, 5), (tc.LEFT, 129), (tc.UP, 3), (tc.LEFT, 64), (tc.DIAGONAL, 30), (tc.UP, 9), (tc.LEFT, 127), (tc.DIAGONAL, 2),
             (tc.LEFT, 3000))
    for code, count in plan2:
        for _ in range(count):
            P[i, j] = code
            i, j = i - (code & 1), j - (code >> 1)
    P[i, j] = tc.NONE
    assert i == 1
    pos1, pos2 = s1[0] * m + s1[1], s2[0] * m + s2[1]
    want1, codes1 = tc.ref_walk_sparse(P, pos1)
    want2, codes2 = tc.ref_walk_sparse(P, pos2)
    _assert_big_path(want1, codes1, m)
    assert len(want2) == sum(c for _, c in plan2) and pos1 * 4 > 2 ** 32 and (want1 // m).min() > 64 > (want2 // m).max()
    d8 = torch.from_numpy(P).to("cuda")
    del P
    dP = engine.widen_p(d8)
    engine.synchronize()
    out = swamd.Fill(H=None, P=dP, res=torch.zeros(3, dtype=torch.int64, device="cuda"), cols=m - 1, rows=rows1 - 1)
    path1 = engine.traceback(out, pos1)
    assert int(out.res[2].item()) == len(want1) and np.array_equal(path1, want1)
    path2 = engine.traceback(out, pos2)
    assert int(out.res[2].item()) == len(want2) and np.array_equal(path2, want2)
    flat8 = d8.view(-1)
    idx = torch.from_numpy(np.concatenate([want1, want2])).to("cuda")
    flat8[idx] = -flat8[idx]
    for r in range(0, rows1, 2048):      # (compared in slices: no second 4 GiB copy)
        assert torch.equal(dP[r:r + 2048], d8[r:r + 2048].to(torch.int32)), f"rows {r}.."


# ---- real fills with long runs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scores", [(3, -3, -2), (10, -1, -1)], ids=["s3", "s10"])
@pytest.mark.parametrize("n", [63, 64, 65, 300])
@pytest.mark.parametrize("side", ["left", "up"])
def test_fill_and_traceback_with_an_insertion(engine, oracle, swamd, side, n, scores):
    """a = X + ins + Y against b = X + Y (and the transpose): X, Y 700 random ACGT letters, ins n letters that occur in neither.  The
    path has 1400 + n cells with one LEFT (resp. UP) run of exactly n -- asserted on the oracle's path before the GPU is looked at."""
    import torch
    rng = np.random.default_rng(1000 * n + scores[0])
    X, Y = (np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 700)] for _ in range(2))
    long, short = np.concatenate([X, np.full(n, ord("N"), np.uint8), Y]), np.concatenate([X, Y])
    a, b = (long, short) if side == "left" else (short, long)
    H, P, mp = oracle.fill(a, b, scores=scores)
    P0 = P.copy()
    opath = oracle.backtrack(P, mp)
    codes = tc.path_codes(P, opath)
    run, other = (tc.LEFT, tc.UP) if side == "left" else (tc.UP, tc.LEFT)
    assert len(opath) == 1400 + n and tc.longest_run(codes, run) == n and (codes == run).sum() == n and (codes == other).sum() == 0
    assert np.array_equal(tc.ref_walk(P0.copy(), mp), opath)
    for p_dtype in (None, torch.int8):
        out = engine.fill(a, b, scores=scores, p_dtype=p_dtype)
        assert out.result()["max_pos"] == mp and np.array_equal(out.P.cpu().numpy().astype(np.int32), P0)
        if p_dtype is torch.int8:
            P2, bits = engine.pack_p2(out.P)
            bits.zero_()
            path2 = engine.traceback_p2(P2, len(a), len(b), mp, bits)
            assert np.array_equal(path2, opath)
            assert np.array_equal(P2.cpu().numpy(), tc.np_pack(P0)[0]) and np.array_equal(bits.cpu().numpy().view(np.uint32), tc.path_bitmap(opath, P0.size))
        path = engine.traceback(out, mp)
        assert out.result()["path_len"] == len(opath) and np.array_equal(path, opath)
        assert np.array_equal(out.P.cpu().numpy().astype(np.int32), P)
