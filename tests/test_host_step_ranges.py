"""Host test of the step epilogue's block ranges (csrc/scn_step_ranges.h): which job a workgroup of scn_step_epilogue runs.

The computation lives in a header without HIP dependencies, so it is checked by a STAND-ALONE program (tests/host_step_ranges_main.cpp,
its own main) built with -fsanitize=address,undefined and run directly -- never loaded into Python.  Per case the program compares
the ranges with brute force (an owner array filled job by job): every block of the grid belongs to exactly one job, with the right
index inside it; every job has as many blocks as its stand-alone launch had; a block outside the grid has none.

Cases: the benchmark's step (two reduces, the first layer's, the readout clear of 128 trajectories, one masked clear of 2048 blocks),
every job absent alone, nothing at all, all caps full, 300 seeded random count vectors, and counts the ranges must refuse (negative; a
grid past 2^30 blocks).  The three grid helpers are compared with the stand-alone launches' own formulas restated here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOBS = 12                                                             # loss, readout_dw, 4 reduces, first, readout clear, 4 masked clears
BENCH = [1, 1, 48, 48, 0, 0, 96, 128, 2048, 0, 0, 0]                   # 3 x 32: (32 * 3 * 32 + 63) // 64 = 48 blocks per reduce


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("step_ranges") / "step_ranges_main")
    # the sanitizer runtimes are linked INTO the program (clang's default; gcc needs telling), as in tests/test_host_visit_records.py
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_rt = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] +
                          static_rt + ["-I" + os.path.join(ROOT, "scone_gcn_amd", "csrc"), os.path.join(ROOT, "tests", "host_step_ranges_main.cpp"),
                                       "-o", exe])
    return exe


def _run(program, tmp_path, cases, helpers=()):
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(np.array([len(cases)], np.int32).tobytes())
        for counts, valid in cases:
            assert len(counts) == JOBS
            f.write(np.array(list(counts) + [int(valid)], np.int64).tobytes())
        f.write(np.array([len(helpers)], np.int32).tobytes())
        for h in helpers:
            f.write(np.array(h, np.int64).tobytes())
    r = subprocess.run([program, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    return r.stdout.strip().split("\n")


def test_every_block_has_exactly_one_job(program, tmp_path):
    rs = np.random.RandomState(5)
    cases = [(BENCH, True), ([0] * JOBS, True), ([1] * JOBS, True)]
    for j in range(JOBS):                                             # each job absent alone
        cases.append(([0 if k == j else c or 3 for k, c in enumerate(BENCH)], True))
    cases.append(([1, 1, 48, 48, 48, 48, 96, 4096, 2048, 2048, 2048, 2048], True))          # five layers, every cap full
    for _ in range(300):
        present = rs.rand(JOBS) < 0.6
        cases.append((list((rs.randint(1, 400, JOBS) * present).astype(int)), True))
    out = _run(program, tmp_path, cases)
    n_blocks = sum(sum(c) for c, _ in cases)
    assert out[0].split() == ["ok", str(len(cases)), str(n_blocks)] and n_blocks > 100000


def test_refused_counts_and_the_stand_alone_grids(program, tmp_path):
    cases = [([1, 1, -1] + [0] * 9, False), ([1 << 30, 1] + [0] * 10, False), ([(1 << 30) + 1] + [0] * 11, False), ([1 << 62] * JOBS, False),
             ([5] + [0] * 11, True)]
    helpers = [(32, 32, 1, 16000), (16, 16, 2, 17), (32, 32, 0, 2048), (1, 1, 1, 2049), (21, 1, 0, 1), (64, 64, 2, 0)]
    out = _run(program, tmp_path, cases, helpers)
    assert out[0].split() == ["ok", str(len(cases)), "5"]
    for line, (c_aux, c_dz, form, nb) in zip(out[1:], helpers):
        # blocked_dw_reduce: one workgroup per 64 outputs; dw_first_reduce: 3 * 32 outputs, the pair form 3 * 16; clear_mask: min(blocks, 2048)
        assert [int(v) for v in line.split()] == [(c_aux * 3 * c_dz + 63) // 64, {0: 0, 1: 96, 2: 48}[form], min(nb, 2048)]
    assert len(out) == 1 + len(helpers)
