#!/usr/bin/env python3
"""Config-3 fixtures from the reference's data file ocean_drifters_data/dataBuoys.jld2 (3.7 MB, HDF5):

* tests/golden/buoy.npz -- the arrays SCoNe needs (edge list, triangle list, hexagon centres, 339 node trajectories);
* tests/golden/dataBuoys_subset.jld2.xz -- the file itself, byte for byte wherever scone_gcn_amd/jld2_reader.py reads it while
  loading those arrays, zeros everywhere else (the other datasets it holds), xz-compressed: the reader's own test input.

    python tests/golden/make_golden_buoy.py <path to ocean_drifters_data/dataBuoys.jld2>

The file is parsed with scone_gcn_amd/jld2_reader.py (h5py is not installed); the conversion rules of the reference's
buoy_data.py are restated in scone_gcn_amd/buoy_data.py and tested against the counts SURVEY.md section 2 records.
"""
import lzma
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from scone_gcn_amd import jld2_reader   # noqa: E402
from scone_gcn_amd.buoy_data import read_buoy_file   # noqa: E402

src = sys.argv[1]
elist, tlist, coords, trajs = read_buoy_file(src)
ptr = np.cumsum([0] + [len(t) for t in trajs]).astype(np.int32)
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "buoy.npz"), elist=elist.astype(np.int16),
                    tlist=tlist.astype(np.int16), coords=coords, traj_ptr=ptr,
                    traj_nodes=np.concatenate([np.asarray(t) for t in trajs]).astype(np.int16))
print("edges", elist.shape, "triangles", tlist.shape, "hexagons", coords.shape, "trajectories", len(trajs))

# ---- the subset of the file the reader touches: record every byte range it indexes, keep those, zero the rest
raw = open(src, "rb").read()
used = np.zeros(len(raw), bool)


class _Touched(bytes):
    def __getitem__(self, k):
        a, e = k.indices(len(self))[:2] if isinstance(k, slice) else (k, k + 1)
        used[a:e] = True
        return bytes.__getitem__(self, k)


_init = jld2_reader.JLD2File.__init__


def _tracked_init(self, path):
    _init(self, path)
    sig = self.buf.find(b"\x89HDF\r\n\x1a\n")
    used[sig:sig + 44] = True                                   # signature .. root object address
    self.buf = _Touched(self.buf)
    self.root_links = self.links(self.root)


jld2_reader.JLD2File.__init__ = _tracked_init
read_buoy_file(src)
jld2_reader.JLD2File.__init__ = _init
subset = np.where(used, np.frombuffer(raw, np.uint8), 0).astype(np.uint8).tobytes()
with tempfile.TemporaryDirectory() as tmp:                     # the subset must read back to the same arrays
    p = os.path.join(tmp, "subset.jld2")
    open(p, "wb").write(subset)
    e2, t2, c2, tr2 = read_buoy_file(p)
assert np.array_equal(e2, elist) and np.array_equal(t2, tlist) and np.array_equal(c2, coords) and tr2 == trajs
out = os.path.join(ROOT, "tests", "golden", "dataBuoys_subset.jld2.xz")
open(out, "wb").write(lzma.compress(subset, preset=9 | lzma.PRESET_EXTREME))
print("subset: %d of %d bytes kept -> %s (%d bytes)" % (int(used.sum()), len(raw), os.path.relpath(out, ROOT), os.path.getsize(out)))
