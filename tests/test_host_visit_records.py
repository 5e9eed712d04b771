"""Host test of the packed per-block records of the block plan (csrc/scn_blk_record.h), which the visiting backwards read a unit's
header from (csrc/scn_blk_bwd.inc, ops.VISIT_RECORDS).

The packing lives in a header without HIP dependencies, so it is checked by a STAND-ALONE program (tests/host_visit_records_main.cpp,
its own main) built with -fsanitize=address,undefined and run directly -- never loaded into Python.  The program packs the records of
every case in a file written here and compares every field, read back as the eight 32-bit words a kernel reads, with the separate
arrays:

  * the hand-built operators of tests/test_host_block_plan_limits.py (`small`, `mixed`, `unhinted`): a 64-row block, one row of 128
    sources at width 128, the 32 x 36 ELL-cap block, the entry-less block, and the 1 / 2 / 7 / 8 / 9 / 63-row blocks -- asserted
    present from the restated cut;
  * 300 seeded heavy-tailed random patterns through the same restated cut;
  * one case whose source count does not fit its byte, which the packing must refuse.

(The touch-ahead of the next unit's ELL lines was measured and taken out -- profiles/visit_records_ab.txt -- so there are no touch
addresses to check.)

The per-wave tile widths of a real plan come out of the layout pass, which the restated cut does not have; the packing only copies
them, so they are seeded bytes here, all sixteen different per block."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_host_block_plan_limits import BK_ELL_CAP, _heavy_tailed, cut_of, restate_cut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arrays(cut, rs):
    """the plan's separate arrays of a restated cut [(row0, rows, sources, width, reason)]"""
    n = len(cut)
    row0 = np.array([b[0] for b in cut], np.int32)
    rows = np.array([b[1] for b in cut], np.uint8)
    src_ptr = np.r_[0, np.cumsum([b[2] for b in cut])].astype(np.int32)
    width = np.array([b[3] for b in cut], np.uint8)
    ell_ptr = (np.r_[0, np.cumsum([b[1] * b[3] for b in cut])][:-1]).astype(np.int32)
    tiles = np.stack([rs.permutation(256)[:16] for _ in range(n)]).astype(np.uint8) if n else np.zeros((0, 16), np.uint8)
    return n, row0, src_ptr, ell_ptr, rows, width, np.ascontiguousarray(tiles[:, :8]), np.ascontiguousarray(tiles[:, 8:])


def _case_bytes(arrays, corrupt=0):
    n = arrays[0]
    return b"".join([np.array([n, corrupt], np.int32).tobytes()] + [np.ascontiguousarray(a).tobytes() for a in arrays[1:]])


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("visit_records") / "visit_records_main")
    # the sanitizer runtimes are linked INTO the program (clang's default; gcc needs telling), as in tests/test_host_cone_unit_list.py
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_rt = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] +
                          static_rt + ["-I" + os.path.join(ROOT, "scone_gcn_amd", "csrc"), os.path.join(ROOT, "tests", "host_visit_records_main.cpp"),
                                       "-o", exe])
    return exe


def _run(program, path):
    r = subprocess.run([program, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    return r.stdout.split()


def test_records_of_the_operators_at_the_plans_limits(program, tmp_path):
    rs = np.random.RandomState(1)
    cases = []
    for name in ("small", "mixed", "unhinted"):
        cut = cut_of(name)
        assert cut is not None
        cases.append(_arrays(cut, rs))
    small = cut_of("small")
    assert any(b[1] == 64 for b in small) and any(b[1:4] == (1, 128, 128) for b in small), "a 64-row block; one row of 128 sources at width 128"
    assert any(b[1] == 32 and b[3] == 36 and b[1] * b[3] == BK_ELL_CAP for b in small) and any(b[3] == 0 for b in small), "the ELL-cap and the entry-less block"
    assert {1, 2, 7, 8, 9, 63} <= {b[1] for b in small}
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(np.array([len(cases)], np.int32).tobytes() + b"".join(_case_bytes(c) for c in cases))
    out = _run(program, path)
    assert out == ["ok", str(len(cases)), str(sum(c[0] for c in cases))]


def test_records_of_seeded_random_patterns_and_a_count_past_its_byte(program, tmp_path):
    rs = np.random.RandomState(11)
    cases = []
    for i in range(300):
        rowptr, col = _heavy_tailed(rs, 130 + i % 50)                 # (a row has up to 126 entries)
        hint = None if i % 3 == 0 else (rs.rand(len(rowptr) - 1) < 0.2).astype(np.uint8)
        cut = restate_cut(rowptr, col, True, hint)
        assert cut is not None
        cases.append(_case_bytes(_arrays(cut, rs)))
    n_blocks = sum(int(np.frombuffer(c[:4], np.int32)[0]) for c in cases)
    bad = list(_arrays([(0, 1, 128, 128, "hint"), (1, 1, 2, 2, "end")], rs))
    bad[2] = np.array([0, 256, 258], np.int32)                       # 256 sources: no plan has such a block, and a byte cannot hold it
    cases.append(_case_bytes(tuple(bad), corrupt=1))
    cases.append(_case_bytes(_arrays([], rs)))                        # no block at all
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(np.array([len(cases)], np.int32).tobytes() + b"".join(cases))
    out = _run(program, path)
    assert out == ["ok", str(len(cases)), str(n_blocks)] and n_blocks > 1000
