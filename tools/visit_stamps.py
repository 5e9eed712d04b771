#!/usr/bin/env python3
"""Diagnostic: where a visit of the two visiting backwards goes, per WORKGROUP -- the unit's prologue (drain + barrier, header and
metadata loads, the first slab's DMA) apart from the visit's own segments (wait, barrier, gather, contraction), from the -DSCN_STAMPS
build (tools/build_stamps.sh).  Tensors, masks and launches are those of tools/window_scan_floor.py.

    python tools/visit_stamps.py [--masks bench] [--top 4]

Prints, for the busiest workgroups of bwd2_first_visit (M2) and bwd3_visit (M1): units, visits, the stamped segments per visit in
s_memtime ticks (mean over the workgroup's eight waves), the share of the prologue in the workgroup's time above the all-zero floor,
and what the launch would take with the prologue hidden: floor + visits x (visit - hidden part)."""
import argparse
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
STAMPS = os.path.join(HERE, "ubench", "libscone_hip_stamps.so")
ap = argparse.ArgumentParser()
ap.add_argument("--masks", default="bench")
ap.add_argument("--top", type=int, default=4)
a = ap.parse_args()
sys.argv = [sys.argv[0], "--masks", "zero," + a.masks, "--rounds", "2", "--reps", "10",
            "--libs", "new=scone_gcn_amd/libscone_hip.so,stamps=" + STAMPS]
sys.path.insert(0, HERE)
import torch                       # noqa: E402
import window_scan_floor as f      # noqa: E402  (builds the tensors and masks, and times the launches of both builds)
from scone_gcn_amd import _lib     # noqa: E402

lib, plan, _ = f.builds["stamps"]
_lib._lib = lib
dbg = ctypes.CDLL(STAMPS)
CAP, WAVES, WORDS = 1024, 8, 16
buf = np.zeros((CAP, WAVES, WORDS), dtype=np.uint64)
ptr = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong))
NAMES = ["wait", "barrier", "gather", "dgrad", "epi+dW", "(a) drain+bar", "(b) header+meta", "issue tw+DMA", "(c) 1st DMA wait", "scan+between"]


def stamped(key, kind):
    fn = f.launches(plan, f.MASKS[kind])[key]
    fn()
    torch.cuda.synchronize()
    assert dbg.scn_debug_stamps_wg(ptr, 1) == 0
    fn()
    torch.cuda.synchronize()
    assert dbg.scn_debug_stamps_wg(ptr, 0) == 0
    return buf.astype(np.float64)


for key in ("bwd2_first_visit", "bwd3_visit"):
    zero = stamped(key, "zero")
    used = zero[:, 0, 15] > 0
    floor = float(np.median(zero[used, :, 15].max(axis=1)))
    us_zero = {n: np.mean(f.times[("zero", key, n)]) for n in f.builds}
    for kind in a.masks.split(","):
        s = stamped(key, kind)
        span = s[:, :, 15].max(axis=1)                       # entry -> exit of the workgroup's slowest wave
        us = {n: np.mean(f.times[(kind, key, n)]) for n in f.builds}
        tick_us = (span.max() - floor) / max(us["stamps"] - us_zero["stamps"], 1e-9)
        print("==== %s, masks %s: %d workgroups; launch %.1f us (product build), %.1f us (stamped build); all-zero %.1f / %.1f us"
              % (key, kind, int(used.sum()), us["new"], us["stamps"], us_zero["new"], us_zero["stamps"]))
        print("     all-zero floor of a workgroup %.0f ticks; slowest workgroup %.0f ticks; %.0f ticks per us above the floor (stamped build)"
              % (floor, span.max(), tick_us))
        print("     launch totals: %d units, %d visits, %d contracted (wave 0)" % (s[:, 0, 10].sum(), s[:, 0, 11].sum(), s[:, 0, 12].sum()))
        for g in np.argsort(-span)[:a.top]:
            w = s[g].mean(axis=0)                            # mean over the eight waves
            units, visits, live = w[10], w[11], s[g, :, 12].mean()
            above = span[g] - floor
            pro = w[5] + w[6] + w[8]
            print("  workgroup %4d: %2d units, %2d visits (%.1f contracted per wave); entry -> exit %.0f ticks, above the floor %.0f = %.0f per visit"
                  % (g, units, visits, live, span[g], above, above / max(visits, 1)))
            print("     per visit: " + "  ".join("%s %.0f" % (n, w[i] / max(visits, 1)) for i, n in enumerate(NAMES)))
            print("     per unit:  (a) %.0f  (b) %.0f  issue %.0f  (c) %.0f  scan+between %.0f" % tuple(w[i] / max(units, 1) for i in (5, 6, 7, 8, 9)))
            print("     (a) + (b) + (c) = %.0f ticks = %.1f %% of the time above the floor; stamped segments cover %.1f %% of entry -> exit"
                  % (pro, 100.0 * pro / max(above, 1), 100.0 * w[:10].sum() / max(span[g], 1)))
            hidden_us = pro / max(tick_us, 1e-9)
            print("     prediction, (a) + (b) + (c) of every unit but the first hidden: %.1f - %.1f = %.1f us (product build's launch)"
                  % (us["new"], hidden_us * (units - 1) / max(units, 1), us["new"] - hidden_us * (units - 1) / max(units, 1)))
