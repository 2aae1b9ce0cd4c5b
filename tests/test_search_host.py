"""CPU: sw_read_fasta_db (every record of a FASTA file in one pass) agrees with sw_read_fasta record by record, and the
ISA audit covers the database-search kernels.  No GPU is needed."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_lib import ROOT

FILES = {
    "mixed": b"; a comment before the first record\n>r0 first\nACGT\nacgt\n\n>r1 empty\n>r2\r\nMKV LA\r\n;inner comment\r\nwxyz\r\n>r3\n\n\n>r4 last\nN",
    "headerless": b"acgtn\nNNNN\n\n;comment\nttt\n",
    "headerless_then_records": b"ACG\n>x\nTT\n>y\n",
    "only_headers": b">a\n>b\n>c\n",
    "crlf_blank": b"\r\n\r\n>one\r\nAC GT\tA\r\n\r\n>two\r\n\r\n",
    "protein": b">p1 some protein\nMKTAYIAKQRQISFVKSHFSRQLEERLGLIEVQAPILSRVGDGTQDNLSGAEKAVQVKVKALPDAQFEVV\nHVAKGQ*\n>p2\nbzx*BZX\n",
}


def _write(tmp_path, name, data):
    p = tmp_path / f"{name}.fa"
    p.write_bytes(data)
    return str(p)


@pytest.mark.parametrize("name", sorted(FILES))
def test_read_fasta_db_matches_per_record_reader(swamd, tmp_path, name):
    path = _write(tmp_path, name, FILES[name])
    seq, offs = swamd.read_fasta_db(path)
    assert offs.dtype == np.int64 and seq.dtype == np.uint8
    assert offs[0] == 0 and np.all(np.diff(offs) >= 0) and offs[-1] == len(seq)
    nrec = len(offs) - 1
    for k in range(nrec):
        assert np.array_equal(seq[offs[k]:offs[k + 1]], swamd.read_fasta(path, k)), f"record {k}"
    with pytest.raises(swamd.SwError):
        swamd.read_fasta(path, nrec)   # the one-pass reader saw every record the per-record reader knows
    # counts-only call
    L = swamd.lib()
    n, t = swamd._i64(), swamd._i64()
    assert L.sw_read_fasta_db(os.fsencode(path), None, 0, None, 0, swamd.ctypes.byref(n), swamd.ctypes.byref(t)) == 0
    assert n.value == nrec and t.value == len(seq)


def test_read_fasta_db_expected_records(swamd, tmp_path):
    seq, offs = swamd.read_fasta_db(_write(tmp_path, "mixed", FILES["mixed"]))
    recs = [bytes(seq[offs[k]:offs[k + 1]]) for k in range(len(offs) - 1)]
    assert recs == [b"ACGTACGT", b"", b"MKVLAWXYZ", b"", b"N"]
    seq, offs = swamd.read_fasta_db(_write(tmp_path, "hl", FILES["headerless"]))
    assert list(offs) == [0, 12] and bytes(seq) == b"ACGTNNNNNTTT"
    seq, offs = swamd.read_fasta_db(_write(tmp_path, "e", b""))
    assert list(offs) == [0] and len(seq) == 0


def test_read_fasta_db_rejects_small_buffers(swamd, tmp_path):
    path = _write(tmp_path, "mixed", FILES["mixed"])
    L = swamd.lib()
    n, t = swamd._i64(), swamd._i64()
    seq = np.zeros(4, np.uint8)
    offs = np.zeros(8, np.int64)
    rc = L.sw_read_fasta_db(os.fsencode(path), seq.ctypes.data, len(seq), offs.ctypes.data, len(offs), swamd.ctypes.byref(n), swamd.ctypes.byref(t))
    assert rc == -22 and b"too small" in L.sw_last_error()
    assert L.sw_read_fasta_db(os.fsencode(str(tmp_path / "missing.fa")), None, 0, None, 0, swamd.ctypes.byref(n), swamd.ctypes.byref(t)) == -22


def test_top_hits_order(swamd):
    res = np.array([[0, 5, 0], [0, 9, 0], [0, 5, 0], [0, 0, 0], [0, 9, 0]], np.int64)
    assert list(swamd.top_hits(res, 3)) == [1, 4, 0]
    assert list(swamd.top_hits(res, 99)) == [1, 4, 0, 2, 3]


def test_check_isa_audits_search_kernels():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_isa.py")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "search kernels without scratch" in out.stdout
