"""CPU: the three host legs that read a hit table's alignments -- sw_pssm_from_hits_host, sw_pssm_hit_weights_host and
sw_msa_from_hits_host -- read it THE SAME WAY.  Each is held to its own restated reference elsewhere; here the same seeded tables
(tests/hit_tables_cases.py: every way of being unused, op rows that run past either end) go through all three, and what they leave
must agree exactly: a column's counts sum to the letters in that column of the column rows, an entry's letters to its nmatch, len is 0
or qlen + ninsert, no pair means no weight, and a query has weight exactly when one of its entries has a pair."""
import hit_tables_cases as hc


def test_the_three_host_legs_agree(swamd):
    kinds = set()
    for seed in hc.SEEDS:
        c = hc.tables(seed)
        assert hc.assert_agree(c, *hc.host_legs(swamd, c)) > 0, seed
        kinds |= set(c.kind.reshape(-1).tolist())
    assert kinds == set(range(hc.UNUSED_KINDS + 1))               # used, and every way of being unused
