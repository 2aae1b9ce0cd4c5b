"""CPU: the batch and search planners (smith-waterman_amd/csrc/sw_plan.cpp), driven through tests/fill_plan_driver.cpp (kind=batch,
kind=search).  Every threshold of the policy from both sides, the kernel of every chunk, the search grid and the schedule.

The search occupancies handed in are illustrative (the real ones are queried from the device once per context); what is checked is
that the grid follows the occupancy of the instantiation the plan picks."""
import json
import subprocess

import pytest

from test_fill_plan import driver  # noqa: F401  (the driver, built once per module)

SINGLE_PAIR, NO_WAVE16, NO_PACKED_P = 1 << 16, 1 << 18, 1 << 21
# The order of kBatch in sw_api_fill.hip (a static_assert there holds every entry to swp::batch_wave_index / batch_wave16_index).
KBATCH = [("wave", 4, 0), ("wave", 4, 1), ("wave", 4, 4), ("wave", 8, 0), ("wave", 8, 1), ("wave", 8, 4), ("wave", 16, 0), ("wave", 16, 1),
          ("wave", 16, 4)] + [("wave16", le4, k12, pb1) for le4 in (0, 1) for k12 in (0, 1) for pb1 in (0, 1)]


def wave(C, pb):
    """index of sw_batch_wave<C, PB> in kBatch"""
    return KBATCH.index(("wave", C, pb))


def wave16(le4, k12, pb1):
    """index of sw_batch_wave16<LE4, K12, PB1> in kBatch"""
    return KBATCH.index(("wave16", le4, k12, pb1))


def run(driver, kind, kw):
    line = f"kind={kind} " + " ".join(f"{k}={int(v) if isinstance(v, bool) else v}" for k, v in kw.items())
    return json.loads(subprocess.run([driver], input=line + "\n", capture_output=True, text=True, check=True).stdout)


@pytest.fixture(scope="module")
def batch(driver):  # noqa: F811
    def plan(**kw):   # score-only 1024^2 pairs with the reference's scores unless told otherwise
        return run(driver, "batch", {"cols": 1024, "rows": 1024, "npairs": 1000, "has_H": 0, "has_P": 0, **kw})
    return plan


@pytest.fixture(scope="module")
def search(driver):  # noqa: F811
    def plan(**kw):
        return run(driver, "search", {"num_cus": 256, "search_per_cu": 8, "qlen": 512, "maxlen": 400, "ntargets": 100000, **kw})
    return plan


def test_batch_eligibility_scores(batch):
    assert batch(match=127, mismatch=-127)["wave"] == 1
    assert batch(match=128, mismatch=-127)["wave"] == 0
    assert batch(match=3, mismatch=-128)["wave"] == 0
    assert batch(debug_flags=SINGLE_PAIR)["wave"] == 0


def test_batch_eligibility_2gib(batch):
    # (rows + 132) x (cols + 1) ints below 2 GiB: 1024 x (rows + 132) x 4 < 2^31
    assert batch(cols=1023, rows=524155, npairs=2)["wave"] == 1
    assert batch(cols=1023, rows=524156, npairs=2)["wave"] == 0


def test_batch_columns_per_lane(batch):
    assert [batch(cols=c)["C"] for c in (1, 256, 257, 512, 513, 1024)] == [4, 4, 8, 8, 16, 16]
    assert (batch(cols=256)["nstrips"], batch(cols=257)["nstrips"]) == (1, 1)
    assert (batch(cols=1024)["nstrips"], batch(cols=1025)["nstrips"], batch(cols=2500)["nstrips"]) == (1, 2, 3)


def test_batch_codes_and_boundary(batch):
    p = batch(rows=1024)
    assert (p["front"], p["per"], p["bnd_per"]) == (64, 1248, 0)   # 1024 + 64 + 80 + 72, whole 16 bytes
    assert batch(rows=1016)["per"] == 1232 and batch(rows=1017)["per"] == 1248
    p = batch(cols=1025, rows=1024)
    assert (p["bnd_per"], p["bnd_need"]) == (1184, 1000 * 1184)   # rows + 160, whole 4 ints
    assert batch(cols=1025, rows=1021)["bnd_per"] == 1184 and batch(cols=1025, rows=1025)["bnd_per"] == 1188
    assert (batch()["bcodes_need"], batch()["bnd_need"]) == (1000 * 1248, 0)


def test_batch_chunk_bounds(batch):
    # 1 GiB of padded codes: 2^30 // 1248 = 860370 pairs
    assert batch(npairs=860370)["chunk"] == 860370
    p = batch(npairs=860371)
    assert (p["chunk"], p["grid"], p["bcodes_need"]) == (860370, 215093, 860370 * 1248)
    # 1 GiB of boundary columns: 2^30 // (1184 * 4) = 226719 pairs
    assert batch(cols=2048, npairs=226719)["chunk"] == 226719
    p = batch(cols=2048, npairs=226720)
    assert (p["chunk"], p["bnd_need"]) == (226719, 226719 * 1184)
    assert batch(npairs=1)["chunk"] == 1 and batch(npairs=1)["grid"] == 1
    assert batch(npairs=5)["grid"] == 2


def test_batch_scan_blocks(batch):
    # one sw_prep_scan block per 4096 letters (a + b of every pair), at least 1, at most 2048
    assert batch(cols=2048, rows=2048, npairs=1)["scan_blocks"] == 1
    assert batch(cols=2048, rows=2049, npairs=1)["scan_blocks"] == 2
    assert batch(npairs=4096)["scan_blocks"] == 2048
    assert batch(npairs=4097)["scan_blocks"] == 2048
    assert batch(npairs=4094)["scan_blocks"] == 2047
    assert batch(rows=1024)["codes_blocks"] == 5 and batch(rows=20000)["codes_blocks"] == 64


def test_batch_packed16_eligibility(batch):
    assert batch()["fits16"] == 1
    assert batch(npairs=1)["fits16"] == 0
    assert batch(cols=512)["fits16"] == 0 and batch(cols=513)["fits16"] == 1   # C == 16
    # match x min(cols, rows) below 32000
    assert batch(cols=1000, rows=1000, match=31)["fits16"] == 1 and batch(cols=1000, rows=1000, match=32)["fits16"] == 0
    assert batch(cols=1032, rows=1032, match=31)["fits16"] == 1 and batch(cols=1033, rows=1033, match=31)["fits16"] == 0
    # -gap below 32000
    assert batch(gap=-31999)["fits16"] == 1 and batch(gap=-32000)["fits16"] == 0
    # fewer than 65000 rows
    assert batch(cols=600, rows=64999)["fits16"] == 1 and batch(cols=600, rows=65000)["fits16"] == 0
    assert batch(debug_flags=NO_WAVE16)["fits16"] == 0


@pytest.mark.parametrize("match,cols,rows,k12", [(3, 1024, 1024, 1), (3, 1365, 1365, 1), (3, 1366, 1366, 0), (4, 1024, 1024, 0),
                                                 (7, 600, 585, 1), (7, 600, 586, 0)])
def test_batch_keyed_argmax_up_to_12_bit_scores(batch, match, cols, rows, k12):
    # (the cases of test_batch_wave_gpu.py::test_packed16_keyed_argmax_up_to_12_bit_scores)
    p = batch(match=match, cols=cols, rows=rows)
    assert (p["k12"], p["fits16"], p["packed16"]) == (k12, 1, 1)


def test_batch_fifteen_bit_fallback(batch):
    # scores of 12 .. 15 bits: two pairs per wave, the descent instead of the keys; beyond 15 bits: one pair per wave
    p = batch(match=20)
    assert (p["k12"], p["packed16"], p["kernel"]) == (0, 1, wave16(1, 0, 0))
    p = batch(match=32)
    assert (p["k12"], p["packed16"], p["kernel"]) == (0, 0, wave(16, 0))


def test_batch_packed16_outputs(batch):
    assert batch()["packed16"] == 1                                          # score-only
    assert batch(has_P=1, p_elem_bytes=1)["packed16"] == 1                   # int8 P as the only matrix
    assert batch(has_P=1, p_elem_bytes=4)["packed16"] == 0
    assert batch(has_H=1)["packed16"] == 0
    assert batch(has_H=1, has_P=1, p_elem_bytes=1)["packed16"] == 0
    assert batch(has_P=1, p_elem_bytes=1, debug_flags=NO_PACKED_P)["packed16"] == 0
    assert batch(debug_flags=NO_PACKED_P)["packed16"] == 1                   # (bit 21 only takes the int8 P)


def test_batch_single_pair_chunks(batch):
    assert [batch(npairs=n)["single_chunk"] for n in (1, 4095, 4096, 4097, 100000)] == [1, 4095, 4096, 4096, 4096]
    assert batch(match=200, npairs=10000)["single_chunk"] == 4096


def test_batch_kernel_pick(batch):
    # more than 8 letters: the fall-back
    assert batch(nletters=8)["kernel"] == wave16(0, 1, 0)
    assert batch(nletters=9)["kernel"] == -1
    assert batch(has_H=1, nletters=9)["kernel"] == -1
    # up to 4 letters: half-size profiles
    assert batch(nletters=4)["kernel"] == wave16(1, 1, 0) and batch(nletters=5)["kernel"] == wave16(0, 1, 0)
    assert batch(nletters=1, has_P=1, p_elem_bytes=1, pb=1)["kernel"] == wave16(1, 1, 1)
    assert batch(nletters=6, match=20, has_P=1, p_elem_bytes=1, pb=1)["kernel"] == wave16(0, 0, 1)
    # one pair per wave: C and the P width
    for cols, C in ((256, 4), (257, 8), (512, 8), (513, 16)):
        assert batch(cols=cols, has_H=1, has_P=1, pb=4)["kernel"] == wave(C, 4)
        assert batch(cols=cols, has_P=1, p_elem_bytes=1, pb=1, debug_flags=NO_WAVE16)["kernel"] == wave(C, 1)
        assert batch(cols=cols, has_H=1, pb=0)["kernel"] == wave(C, 0)


def test_batch_kernel_of_an_odd_last_chunk(batch):
    # wave16 chunks, then one pair left: sw_batch_wave<16, PB> (last_batch_kernel still reports 2)
    assert batch(n=2)["kernel"] == wave16(1, 1, 0)
    assert batch(n=1)["kernel"] == wave(16, 0)
    assert batch(n=1, has_P=1, p_elem_bytes=1, pb=1)["kernel"] == wave(16, 1)


def test_search_columns_per_lane_and_profile(search):
    assert [search(qlen=q)["C"] for q in (1, 256, 257, 512, 513, 4096)] == [4, 4, 8, 8, 16, 16]
    p = search(qlen=1024)
    assert (p["nstrips"], p["qpad"], p["bnd_per"], p["prof_need"], p["prof_blocks"]) == (1, 1024, 0, 257 * 1024, 1028)
    p = search(qlen=1025, maxlen=1024)
    assert (p["nstrips"], p["qpad"], p["bnd_per"]) == (2, 2048, 1184)
    assert search(qlen=256)["qpad"] == 256 and search(qlen=257)["qpad"] == 512
    assert search(qlen=3072)["prof_blocks"] == 3084 and search(qlen=4096)["prof_blocks"] == 4096   # at most 4096 blocks


def test_search_wide_scores(search):
    assert search(match=127, mismatch=-127)["wide"] == 0
    assert search(match=128, mismatch=-127)["wide"] == 1
    assert search(match=3, mismatch=-128)["wide"] == 1
    # kernel index 2 * (C / 8) + wide
    assert [search(qlen=q, match=m)["kernel"] for q, m in ((256, 3), (256, 200), (512, 3), (512, 200), (513, 3), (513, 200))] == [0, 1, 2, 3, 4, 5]


def test_search_grid(search):
    # as many workgroups as are resident, of the instantiation picked
    assert search()["grid"] == 8 * 256
    assert search(search_per_cu="1,2,3,4,5,6")["grid"] == 3 * 256
    assert search(qlen=513, match=200, search_per_cu="1,2,3,4,5,6")["grid"] == 6 * 256
    # ... or one per 4 targets
    assert search(ntargets=8192)["grid"] == 2048 and search(ntargets=8189)["grid"] == 2048
    assert search(ntargets=8188)["grid"] == 2047 and search(ntargets=1)["grid"] == 1
    # boundary columns of a multi-strip query (one per wave, rows + 160 of the longest target) below 1 GiB: 2^30 // (bnd_per * 16)
    p = search(qlen=1025, maxlen=32608)
    assert (p["bnd_per"], p["grid"], p["bnd_need"]) == (32768, 2048, 2048 * 4 * 32768)
    p = search(qlen=1025, maxlen=32609)
    assert (p["bnd_per"], p["grid"], p["bnd_need"]) == (32772, 2047, 2047 * 4 * 32772)
    assert search(qlen=1025, maxlen=1000000)["grid"] == 67
    assert search(qlen=1024, maxlen=1000000)["grid"] == 2048   # one strip: no boundary columns


def test_search_schedule(search):
    # empty targets dropped, decreasing length, ties in input order: {start, index, length}
    p = search(ntargets=6, offsets="0,3,3,5,8,12,14,17")
    assert p["items"] == [[8, 4, 4], [0, 0, 3], [5, 3, 3], [14, 6, 3], [3, 2, 2], [12, 5, 2]]
    # ties among many items (a short std::sort would be an insertion sort, stable by accident): 40 targets of lengths 1, 2, 3, 1, 2, ...
    lens = [1 + k % 3 for k in range(40)]
    offsets = [0]
    for n in lens:
        offsets.append(offsets[-1] + n)
    p = search(ntargets=40, offsets=",".join(map(str, offsets)))
    assert p["items"] == [[offsets[k], k, lens[k]] for k in sorted(range(40), key=lambda k: -lens[k])]
    assert search(offsets="0,0,0")["items"] == []
    assert search(offsets="5,6,7,8,9")["items"] == [[5, 0, 1], [6, 1, 1], [7, 2, 1], [8, 3, 1]]
