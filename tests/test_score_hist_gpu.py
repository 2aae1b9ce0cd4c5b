"""GPU: the score histogram on the device (sw_score_hist_device) against its host leg, byte for byte, on synthetic result tables over
a real handle (the kernel reads the handle's offsets, never the letters, so the handle's bytes are one zero): 1, 63, 64, 65, 257 and
5000 targets -- slices and their tails --, 1, 3 and 70 queries, every target of a query in ONE cell (5000 adds to one counter) and the
scores spread over all 256 bins, the class edges with shifts 0, 3 and 16, empty targets, one target of 2^20 - 1 letters, the table and
the histogram at odd element bases inside poisoned guards that come back intact, 1, 2 and 4 LDS copies, twice on one stream the same
bytes; the refusals and the empty calls."""
import numpy as np
import pytest

import score_stats_cases as sc

pytestmark = pytest.mark.gpu

G = sc.GUARD


def handle(engine, offs):
    t = engine.torch
    return engine.prepare_db(t.zeros(1, dtype=t.uint8, device=f"cuda:{engine.device}"), offs)


def device_leg(engine, db, res, shift, odd=1):
    """One call: the table `odd` int64 elements and the histogram `odd` counters off their allocations, both between poisoned guards."""
    t, dev = engine.torch, f"cuda:{engine.device}"
    nq, n = res.shape[0], res.size
    tab = t.full((G + odd + n + G,), sc.P64, dtype=t.int64, device=dev)
    tab[G + odd:G + odd + n] = t.from_numpy(res.reshape(-1).copy()).to(dev)
    before = tab.clone()
    hist = t.full((G + odd + nq * sc.CELLS + G,), sc.P32, dtype=t.int32, device=dev)
    out = engine.score_hist_device(db, tab[G + odd:G + odd + n], nq, shift, hist=hist[G + odd:G + odd + nq * sc.CELLS])
    engine.synchronize()
    assert (tab == before).all().item()                                       # the table is only read
    h = hist.cpu().numpy()
    assert (h[:G + odd] == sc.P32).all() and (h[G + odd + nq * sc.CELLS:] == sc.P32).all()
    return out.cpu().numpy().view(np.uint32)


def equal_to_host(swamd, engine, res, offs, shift, odd=1):
    exp = swamd.score_hist_host(res, offs, shift)
    with handle(engine, offs) as db:
        got = device_leg(engine, db, res, shift, odd)
        assert got.shape == exp.shape and (got == exp).all(), int((got != exp).sum())
        assert (device_leg(engine, db, res, shift, odd + 2) == got).all()     # once more: the same bytes
    return got


@pytest.mark.parametrize("ntargets", [1, 63, 64, 65, 257, 5000])
@pytest.mark.parametrize("nq", [1, 3, 70])
def test_random_tables_equal_the_host_leg(swamd, engine, ntargets, nq):
    rng = np.random.default_rng(ntargets * 100 + nq)
    lens = np.clip(np.exp(rng.normal(5, 0.8, ntargets)).astype(np.int64), 0, 3000)
    lens[rng.random(ntargets) < 0.05] = 0
    offs = sc.offsets_of(lens, first=11)
    res = sc.table(rng.integers(-3, 300, (nq, ntargets)))
    got = equal_to_host(swamd, engine, res, offs, 0)
    assert (got.sum(axis=(1, 2)) == (lens > 0).sum()).all()
    assert engine.get_option("last_score_hist_launches") == (1 if ntargets else 0)
    if ntargets == 5000 and nq == 1:
        assert engine.get_option("last_score_hist_slices") == 1               # below 2 x 4096 targets: one slice


def test_one_cell_and_all_bins(swamd, engine):
    offs = sc.offsets_of([150] * 5000)
    one_cell = sc.table(np.full((3, 5000), 41))
    got = equal_to_host(swamd, engine, one_cell, offs, 0)
    assert (got[:, sc.length_class(150), 41] == 5000).all() and (got.sum(axis=(1, 2)) == 5000).all()
    spread = sc.table(np.arange(3 * 5000).reshape(3, 5000) % 256)
    got = equal_to_host(swamd, engine, spread, offs, 0)
    assert (got[:, sc.length_class(150), :] > 0).all()


def test_several_slices_per_query(swamd, engine):
    """25 000 targets: 6 slices of 4167 for a query alone, with a tail of 4165."""
    rng = np.random.default_rng(25)
    lens = rng.integers(0, 41, 25000)
    offs = sc.offsets_of(lens)
    res = sc.table(rng.integers(0, 80, (2, 25000)))
    equal_to_host(swamd, engine, res, offs, 0)
    assert engine.get_option("last_score_hist_slices") == 6
    res[:, :, 1] = 17                                                         # every slice adds to the same few counters
    equal_to_host(swamd, engine, res, offs, 0)


@pytest.mark.parametrize("copies", [1, 2, 4])
def test_lds_copies_write_the_same_bytes(swamd, engine, copies):
    rng = np.random.default_rng(4)
    lens = rng.integers(0, 600, 9000)
    offs = sc.offsets_of(lens)
    res = sc.table(rng.integers(0, 120, (3, 9000)))
    assert engine.get_option("score_hist_copies") == 0
    with pytest.raises(swamd.SwError):
        engine.set_option("score_hist_copies", 3)
    engine.set_option("score_hist_copies", copies)
    try:
        equal_to_host(swamd, engine, res, offs, 0)
    finally:
        engine.set_option("score_hist_copies", 0)


@pytest.mark.parametrize("shift", sc.SHIFTS)
def test_class_edges_and_shifts(swamd, engine, shift):
    res, offs = sc.edge_case(shift)
    got = equal_to_host(swamd, engine, res, offs, shift)
    assert (got == sc.hist_ref(res, offs, shift)).all()
    assert (got[:, 39].sum(axis=1) > 0).all()                                 # 2^20 - 1 letters: class 39


def test_one_longest_target(swamd, engine):
    offs = sc.offsets_of([(1 << 20) - 1], first=3)
    got = equal_to_host(swamd, engine, sc.table([[(1 << 24) - 1], [0]]), offs, 16)
    assert got[0, 39, 255] == 1 and got[1, 39, 0] == 1 and got.sum() == 2


def test_refusals_and_the_empty_calls(swamd, engine):
    t, dev = engine.torch, f"cuda:{engine.device}"
    L = swamd.lib()
    res, offs = sc.edge_case(0, nq=2)
    d_res = t.from_numpy(res.reshape(-1).copy()).to(dev)
    hist = t.full((2 * sc.CELLS,), sc.P32, dtype=t.int32, device=dev)

    def untouched():
        engine.synchronize()
        return (hist == sc.P32).all().item()
    with handle(engine, offs) as db, handle(engine, offs[:1]) as empty:
        a = dict(ctx=engine._h, db=db._h, res=d_res.data_ptr(), nq=2, shift=0, hist=hist.data_ptr())
        for over in (dict(ctx=None), dict(db=None), dict(res=None), dict(hist=None), dict(nq=-1), dict(shift=-1), dict(shift=17)):
            assert L.sw_score_hist_device(*{**a, **over}.values(), None) == -22 and untouched(), over
            assert b"sw_score_hist_device" in L.sw_last_error()
        assert L.sw_score_hist_device(*{**a, "nq": 0}.values(), None) == 0 and untouched() and engine.get_option("last_score_hist_launches") == 0
        assert L.sw_score_hist_device(*{**a, "db": empty._h}.values(), None) == 0         # no target: only zeroes
        engine.synchronize()
        assert (hist == 0).all().item() and engine.get_option("last_score_hist_launches") == 0
        assert L.sw_score_hist_device(*a.values(), None) == 0
        engine.synchronize()
        assert (hist.cpu().numpy().view(np.uint32).reshape(2, sc.CLASSES, sc.BINS) == sc.hist_ref(res, offs, 0)).all()
