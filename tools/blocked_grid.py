"""launch_grid of csrc/scn_blk_dispatch.inc restated for the tools that walk a launch's workgroups (scn_window_scan_probe takes the
grid from its caller; the library exports no query for it).  ONE restatement: when the dispatch heuristic changes, change it here."""


def launch_grid(n_blocks, n_slabs, per_cu, n_cus=256):
    """(grid.x, grid.y) of a blocked launch over n_blocks plan blocks and n_slabs slabs at per_cu workgroups per compute unit
    (forward-side gathers 2, the MFMA launches and both backwards 1)."""
    cap, nb_xcd, best, gy = n_cus * per_cu, (n_blocks + 7) // 8, None, 1
    while gy <= 32 and gy <= max(1, n_slabs):
        gx = max(8, min(cap // gy, (n_blocks + 7) // 8 * 8) // 8 * 8)
        cost = ((nb_xcd + gx // 8 - 1) // (gx // 8)) * (2 * ((n_slabs + gy - 1) // gy) + 1) * 64 + gy
        if best is None or cost < best[0]:
            best = (cost, gx, gy)
        gy *= 2
    return best[1], best[2]
