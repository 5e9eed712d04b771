"""The integer arithmetic of a mask's unit list (scone_gcn_amd/csrc/scn_keep_bits.h) without a GPU.

With ops.CONE_UNIT_LIST the forward-side masked launches take their units from a list of the mask's non-empty words: an entry is
block * words + word (unit_block / unit_word take it apart), and the window of an entry is the block's 64-bit window cut to the launch's
slab range (keep_cut) and restricted to the slabs of the entry's word (keep_word_cut) -- a block with bits in two words of a window is
two entries, and every item must come out exactly once.  The functions are compiled here as a stand-alone host program under the
address and undefined-behaviour sanitizers and compared with brute force over the bits: every words-per-block count 1 .. 5, window
starts inside and on word boundaries (the kernels use 0; the helper is written for any), every range length that ends on, before or
after a word boundary.  The program runs as a subprocess; nothing is loaded into Python."""
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

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint64_t rng() {                       // splitmix64, seeded above
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static long checked = 0;
static int failures = 0;

// the window of `row` (bit s = slab s of a block, words * 32 slabs) from slab `first` on: bit j = slab first + j
static uint64_t window(const std::vector<uint32_t>& row, int first) {
    uint64_t win = 0;
    for (int j = 0; j < 64; ++j) {
        const int s = first + j;
        if (s < (int)row.size() * 32 && ((row[s >> 5] >> (s & 31)) & 1)) win |= 1ull << j;
    }
    return win;
}

// one block row at one (first, n): the entries of its non-empty words cover every set bit of the cut window exactly once
static void check(const std::vector<uint32_t>& row, int block, int first, int n) {
    const int words = (int)row.size();
    const uint64_t cut = scn::keep_cut(window(row, first), n);
    uint64_t seen = 0;
    bool ok = true;
    for (int w = 0; w < words; ++w) {
        const uint32_t entry = (uint32_t)block * (uint32_t)words + (uint32_t)w;
        ok = ok && scn::unit_block(entry, words) == block && scn::unit_word(entry, words) == w;
        const uint64_t part = scn::keep_word_cut(cut, first, w);
        for (int j = 0; j < 64; ++j) {                       // brute force: bit j of the cut window, if its slab lies in word w
            const bool want = ((cut >> j) & 1) && ((first + j) >> 5) == w;
            ok = ok && (((part >> j) & 1) == (want ? 1u : 0u));
        }
        ok = ok && (seen & part) == 0;                       // no item twice
        seen |= part;
        if (row[w] == 0) ok = ok && part == 0;               // an empty word (no entry in the list) holds no item
    }
    ok = ok && seen == cut;                                  // every item once
    ++checked;
    if (!ok && ++failures <= 10) std::printf("FAIL words %d block %d first %d n %d\n", words, block, first, n);
}

int main() {
    const int firsts[8] = {0, 1, 31, 32, 33, 63, 64, 100};
    const int lens[9] = {1, 2, 31, 32, 33, 40, 63, 64, 5};
    const int blocks[4] = {0, 1, 16556, 429496729};          // (the last: block * words + word near 2^32 at five words)
    for (int words = 1; words <= 5; ++words)
        for (int first : firsts) {
            if (first >= words * 32) continue;
            for (int n : lens)
                for (int block : blocks) {
                    if ((uint64_t)block * words + words > 0xffffffffull) continue;
                    std::vector<uint32_t> row(words);
                    for (auto& w : row) w = 0;
                    check(row, block, first, n);                                     // empty
                    for (auto& w : row) w = 0xffffffffu;
                    check(row, block, first, n);                                     // full
                    for (int w = 0; w < words; ++w) {                                // bits in exactly one word
                        for (auto& v : row) v = 0;
                        row[w] = (uint32_t)rng() | 1u;
                        check(row, block, first, n);
                        row[w] = 0x80000001u;                                        // the word's two end bits
                        check(row, block, first, n);
                    }
                    for (int r = 0; r < 40; ++r) {
                        for (auto& v : row) v = (uint32_t)(rng() & rng());           // sparse random, some words empty
                        if (r & 1) row[rng() % words] = 0;
                        check(row, block, first, n);
                    }
                }
        }
    std::printf("checked %ld rows, %d failures\n", checked, failures);
    return failures ? 1 : 0;
}
"""


def test_unit_list_helpers_against_brute_force_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "unit_list.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "unit_list"
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
    assert "checked" in r.stdout and r.stdout.strip().endswith(", 0 failures"), r.stdout
    assert int(r.stdout.split("checked ")[1].split()[0]) > 50000, r.stdout
