"""GPU: the low-complexity mask on the device (sw_db_mask_low_complexity) against its host leg, byte for byte and count for count: every
hand-made target of tests/mask_cases.py in one database, at dword-aligned and odd bases and with the output one byte off the input's
alignment; the exact entropy boundaries; windows 2 and 64; a database laid out against the tile borders ("mask_tile": runs across one
and three borders, whole tiles inside a run, triggers far left and far right of the borders they decide, runs and targets that end or
start exactly on a border); runs of hundreds of tiles, so that the carry launch's threads take several tiles each; a database of
empty targets; 2000 random targets of 0..3000 letters.  The output lies in poison between guard bytes, as do the counts; two calls give
the same bytes, a call with another window straight after sees nothing of the one before; the refusals."""
import ctypes

import numpy as np
import pytest

import mask_cases as mc

pytestmark = pytest.mark.gpu

G = mc.GUARD
P64 = 0x5555555555555555


def device_leg(engine, packed, offs, shift=0, want_counts=True, **p):
    """One call on a fresh handle over `packed`: the output pre-filled with poison, `shift` bytes off the input's alignment, the
    counts between guard words.  Returns (out, nmasked) as numpy after checking the guards and the input."""
    t, dev = engine.torch, f"cuda:{engine.device}"
    nt = len(offs) - 1
    d_in = t.from_numpy(packed.copy()).to(dev)
    obuf = t.full((G + shift + len(packed) + G,), 0x5A, dtype=t.uint8, device=dev)
    d_out = obuf[G + shift:G + shift + len(packed)]
    assert (d_out.data_ptr() - d_in.data_ptr()) % 4 == shift % 4
    cbuf = t.full((G + nt + G,), P64, dtype=t.int64, device=dev)
    with engine.prepare_db(d_in, offs) as db:
        db.mask_low_complexity_device(out=d_out, nmasked=cbuf[G:G + nt] if want_counts else False, **mc.params(**p))
        letters = int(offs[-1] - offs[0])
        assert engine.get_option("last_mask_tiles") == -(-letters // engine.get_option("mask_tile"))
        assert engine.get_option("last_mask_launches") == (3 if letters else 0) + (1 if want_counts and nt else 0)
        engine.synchronize()
    obuf, cbuf = obuf.cpu().numpy(), cbuf.cpu().numpy()
    out = obuf[G + shift:G + shift + len(packed)]
    b, e = int(offs[0]), int(offs[-1])
    assert (obuf[:G + shift + b] == 0x5A).all() and (obuf[G + shift + e:] == 0x5A).all()        # nothing outside the range is written
    assert (cbuf[:G] == P64).all() and (cbuf[G + nt:] == P64).all() and (want_counts or (cbuf == P64).all())
    assert np.array_equal(d_in.cpu().numpy(), packed)                                             # the input is only read
    return out, cbuf[G:G + nt] if want_counts else None


def agree(engine, swamd, packed, offs, shift=0, **p):
    out, n = device_leg(engine, packed, offs, shift, **p)
    ref, nref = swamd.mask_low_complexity_host((packed, offs), out=np.full(len(packed), 0x5A, np.uint8), **mc.params(**p))
    assert np.array_equal(n, nref)
    assert np.array_equal(out, ref)
    return out, n


@pytest.mark.parametrize("first,shift", [(0, 0), (64, 0), (77, 0), (0, 1), (3, 3)])
def test_hand_made_targets(engine, swamd, first, shift):
    packed, offs = mc.hand_database(first=first)
    out, n = agree(engine, swamd, packed, offs, shift)
    assert n.sum() > 100
    agree(engine, swamd, packed, offs, shift, mask_byte=ord("A"))


def test_exact_boundaries(engine, swamd):
    for counts, k in (([6, 6], 1000), ([4, 3, 2, 2, 1], 2189)):
        packed, offs = mc.pack([mc.composed(counts), b"", mc.composed(counts)[::-1]])
        for k1, k2, want in ((k, k, 12), (k - 1, k - 1, 0), (k, 5000, 12), (k - 1, 5000, 0)):
            _, n = agree(engine, swamd, packed, offs, trigger_mbits=k1, extend_mbits=k2)
            assert n.tolist() == [want, 0, want]
    packed, offs = mc.pack([b"C" * 12])
    assert agree(engine, swamd, packed, offs, trigger_mbits=0, extend_mbits=0)[1][0] == 12


@pytest.mark.parametrize("W", [2, 64])
def test_window_sizes(engine, swamd, W):
    targets = [t for ts in mc.hand_targets(W).values() for t in ts] + mc.random_targets(60, 0, 300, seed=W, skewed=True)
    packed, offs = mc.pack(targets)
    agree(engine, swamd, packed, offs, window=W)
    targets = mc.random_targets(60, 0, 300, seed=W + 1, skewed=True, alphabet=b"ACD")
    packed, offs = mc.pack(targets, first=5, tail=G)
    k1, k2 = {2: (0, 0), 64: (1300, 1500)}[W]          # over three letters, bounds under which some letters are masked and some are not
    _, n = agree(engine, swamd, packed, offs, window=W, trigger_mbits=k1, extend_mbits=k2)
    assert 0 < n.sum() < int(offs[-1] - offs[0])


@pytest.mark.parametrize("first,shift", [(0, 0), (1, 0)])
def test_tile_borders(engine, swamd, first, shift):
    T = engine.get_option("mask_tile")
    targets, notes = mc.tile_database(T)
    packed, offs = mc.pack(targets, first=first, tail=G if first else 0)
    assert int(offs[-1] - offs[0]) > 14 * T and int(offs[3] - offs[0]) == 5 * T
    out, n = agree(engine, swamd, packed, offs, shift)
    body = out[first:]
    X = ord("X")
    for name in ("across one", "ends on border", "masked to border", "starts on border", "trigger left", "trigger right"):
        pos, L = notes[name]
        assert (body[pos:pos + L] == X).all() and body[pos - 1] == ord("*") and body[pos + L] == ord("*"), name
    pos, L = notes["no trigger"]
    assert (body[pos:pos + L] != X).all()
    # the runs named above sit where they are meant to
    assert notes["across one"][0] < T < sum(notes["across one"]) and sum(notes["ends on border"]) - 12 == 2 * T - 1
    assert sum(notes["masked to border"]) == 3 * T and notes["starts on border"][0] == 4 * T
    assert notes["trigger left"][0] < 6 * T and sum(notes["trigger left"]) > 8 * T
    assert notes["trigger right"][0] < 9 * T and sum(notes["trigger right"]) > 11 * T


def test_runs_of_hundreds_of_tiles(engine, swamd):
    # more than 1024 tiles, so every thread of the carry launch joins several; the runs cross hundreds of tiles, and whole shares
    T = engine.get_option("mask_tile")
    L = 900_000
    targets = [mc._stretch("<", L), mc._stretch("5", L), mc._stretch(">", L), mc._stretch("5", L // 2) + b"*" + mc._stretch(">", L // 2)]
    targets += mc.random_targets(500, 0, 3000, seed=3, skewed=True)
    packed, offs = mc.pack(targets)
    assert int(offs[-1]) > 1025 * T
    out, n = agree(engine, swamd, packed, offs)
    assert n[:4].tolist() == [L, 0, L, L // 2]


def test_all_targets_empty(engine, swamd):
    packed, offs = mc.pack([b""] * 5, first=9, tail=G)
    out, n = agree(engine, swamd, packed, offs)
    assert n.tolist() == [0] * 5
    packed, offs = mc.pack([b""] * 700, tail=G)
    assert agree(engine, swamd, packed, offs)[1].sum() == 0
    device_leg(engine, packed, offs, want_counts=False)


def test_random_targets(engine, swamd):
    targets = mc.random_targets(1000, 0, 3000, seed=21) + mc.random_targets(1000, 0, 3000, seed=22, skewed=True)
    order = np.random.default_rng(23).permutation(len(targets))
    packed, offs = mc.pack([targets[i] for i in order])
    out, n = agree(engine, swamd, packed, offs)
    assert 0.05 < n.sum() / int(offs[-1]) < 0.95
    device_leg(engine, packed, offs, want_counts=False)


def test_repeat_calls_and_another_window(engine, swamd):
    t, dev = engine.torch, f"cuda:{engine.device}"
    targets = mc.random_targets(300, 0, 2000, seed=31, skewed=True)
    packed, offs = mc.pack(targets)
    d_in = t.from_numpy(packed.copy()).to(dev)
    with engine.prepare_db(d_in, offs) as db:
        a, na = db.mask_low_complexity()
        b, nb = db.mask_low_complexity()
        c, nc = db.mask_low_complexity(window=5, trigger_mbits=1000, extend_mbits=1400)
        d, nd = db.mask_low_complexity()
        engine.synchronize()
        assert t.equal(a, b) and t.equal(na, nb) and t.equal(a, d) and t.equal(na, nd)
        ref, nref = swamd.mask_low_complexity_host((packed, offs), window=5, trigger_mbits=1000, extend_mbits=1400)
        assert np.array_equal(c.cpu().numpy(), ref) and np.array_equal(nc.cpu().numpy(), nref)
        ref, nref = swamd.mask_low_complexity_host((packed, offs))
        assert np.array_equal(a.cpu().numpy(), ref) and np.array_equal(na.cpu().numpy(), nref)
    # a smaller database straight after a larger one: the workspace keeps the larger one's bits, none of them is seen
    packed, offs = mc.hand_database()
    agree(engine, swamd, packed, offs)


def test_refusals(engine, swamd):
    t, dev = engine.torch, f"cuda:{engine.device}"
    packed, offs = mc.hand_database()
    d_in = t.from_numpy(packed.copy()).to(dev)
    out = t.full_like(d_in, 0x5A)
    with engine.prepare_db(d_in, offs) as db:
        with pytest.raises(Exception, match="in place"):
            db.mask_low_complexity_device(out=d_in)
        for kw in (dict(window=1), dict(window=65), dict(trigger_mbits=-1), dict(trigger_mbits=2600), dict(extend_mbits=1 << 62), dict(letters=b""),
                   dict(letters=b"ACDA")):
            with pytest.raises(Exception, match="sw_db_mask_low_complexity"):
                db.mask_low_complexity_device(out=out, **mc.params(**kw))
        lib = swamd.lib()
        mp = swamd._mask_params()
        assert lib.sw_db_mask_low_complexity(engine._h, db._h, None, out.data_ptr(), None, engine._stream()) == -22
        assert lib.sw_db_mask_low_complexity(engine._h, db._h, ctypes.byref(mp), None, None, engine._stream()) == -22
        assert lib.sw_db_mask_low_complexity(engine._h, None, ctypes.byref(mp), out.data_ptr(), None, engine._stream()) == -22
        assert lib.sw_db_mask_low_complexity(None, db._h, ctypes.byref(mp), out.data_ptr(), None, engine._stream()) == -22
        engine.synchronize()
        assert (out == 0x5A).all()                       # refused before any launch
