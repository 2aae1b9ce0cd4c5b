"""GPU: the twin of tests/test_hit_tables_agree_host.py.  The same seeded tables go through the three device calls that read them --
sw_db_pssm_from_hits, sw_db_pssm_hit_weights and sw_db_msa_from_hits --; what they leave equals the host legs' byte for byte, and so
agrees among the three in the same way."""
import numpy as np
import pytest

import hit_tables_cases as hc

pytestmark = pytest.mark.gpu


def test_the_three_device_calls_agree_with_the_host_legs(swamd, engine):
    for seed in hc.SEEDS:
        c = hc.tables(seed)
        exp = hc.host_legs(swamd, c)
        prior = (np.zeros((int(c.qoffs[-1]), len(hc.LETTERS)), np.int8), c.qoffs)
        with engine.prepare_db((c.packed, c.offs)) as db:
            _, counts = db.pssm_from_hits(prior, hc.SCORING, (swamd.submat_match(2, -3), 1, c.include_min), c.hits, c.nhits, c.aln, c.ops, want_counts=True)
            weights = db.pssm_hit_weights(hc.SCORING, (hc.PER_HIT, c.include_min), c.qoffs, c.hits, c.nhits, c.aln, c.ops)
            cols, rows, _ = db.msa_from_hits(c.qoffs, c.include_min, c.hits, c.nhits, c.aln, c.ops)
        got = (counts, weights, cols, rows)
        for name, g, e in zip(("counts", "weights", "cols", "rows"), got, exp):
            assert g.dtype == e.dtype and g.tobytes() == e.tobytes(), (seed, name)
        assert hc.assert_agree(c, *got) > 0, seed
