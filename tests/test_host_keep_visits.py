"""The bit arithmetic of the kept forward's visit sequence (scone_gcn_amd/csrc/scn_keep_bits.h) without a GPU.

fwd_c32_w16_kernel<KEEP> runs a block's slab loop over the set bits of its 64-bit keep window: the window is cut to the workgroup's
slab range (keep_cut), its set bits are counted (keep_count) and walked in ascending order with a cursor (keep_first / keep_next).
The same functions are compiled here as a stand-alone host program under the address and undefined-behaviour sanitizers and compared
with brute force over the bits, for every range length 1 .. 64 -- length 64 is the one where a mask written as (1 << n) - 1 shifts by
the type's width.  The program runs as a subprocess; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <vector>
#include "scn_keep_bits.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {                       // splitmix64, seeded above
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static long checked = 0;
static int failures = 0;

// one window at one range length against brute force over the bits
static void check(uint64_t win, int n) {
    std::vector<int> want;
    for (int j = 0; j < n; ++j)
        if ((win >> j) & 1) want.push_back(j);
    const uint64_t cut = scn::keep_cut(win, n);
    bool ok = true;
    for (int j = 0; j < 64; ++j) ok = ok && (((cut >> j) & 1) == (j < n ? ((win >> j) & 1) : 0));
    ok = ok && scn::keep_count(cut) == (int)want.size();
    uint64_t w = cut;
    for (size_t i = 0; i < want.size() && ok; ++i) {
        ok = w != 0 && scn::keep_first(w) == want[i];
        // the cursor one and two visits ahead, as the contraction derives them
        const uint64_t w1 = scn::keep_next(w), w2 = scn::keep_next(w1);
        if (i + 1 < want.size()) ok = ok && w1 != 0 && scn::keep_first(w1) == want[i + 1]; else ok = ok && w1 == 0;
        if (i + 2 < want.size()) ok = ok && w2 != 0 && scn::keep_first(w2) == want[i + 2]; else ok = ok && w2 == 0;
        w = w1;
    }
    ok = ok && (want.empty() ? cut == 0 : w == 0);
    ++checked;
    if (!ok && ++failures <= 10) std::printf("FAIL window %016llx range %d\n", (unsigned long long)win, n);
}

int main() {
    for (int n = 1; n <= 64; ++n) {
        const uint64_t in_range = ~0ull >> (64 - n);
        check(0ull, n);                                      // empty
        check(~0ull, n);                                     // full (and bits above the range wherever n < 64)
        check(in_range, n);                                  // full inside, nothing above
        check(~in_range, n);                                 // nothing inside, everything above
        const int singles[5] = {0, n - 1, 31, 32, 63};
        for (int s : singles) {
            check(1ull << s, n);                             // (a single bit at or above n: outside the range, ignored)
            check((1ull << s) | ~in_range, n);
        }
        check(0x5555555555555555ull, n);                     // alternating, both phases
        check(0xAAAAAAAAAAAAAAAAull, n);
        for (int r = 0; r < 300; ++r) {
            const uint64_t a = rng(), b = rng(), c = rng();
            check(a, n);                                     // dense random, bits above the range included
            check(a & b & c, n);                             // sparse random
            check((a & in_range) | (b & ~in_range), n);      // independent bits above the range
            check(a & b & c & in_range, n);                  // nothing above
        }
    }
    std::printf("checked %ld windows, %d failures\n", checked, failures);
    return failures ? 1 : 0;
}
"""


def test_visit_sequence_helpers_against_brute_force_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "keep_visits.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "keep_visits"
    # the sanitizer runtimes are linked INTO the program (clang's default; gcc needs telling): the program then runs the same
    # whatever else the environment loads ahead of it
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_rt = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined,address",
                           "-fno-sanitize-recover=all"] + static_rt +
                          ["-I" + os.path.join(ROOT, "scone_gcn_amd", "csrc"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    # 64 lengths x (4 + 10 + 2 + 1200) windows
    assert r.stdout.strip().endswith("checked %d windows, 0 failures" % (64 * 1216)), r.stdout
