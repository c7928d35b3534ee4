"""The inpaint rule once more, pixel by pixel in plain Python: the sentences of include/vs_amd.h (vs_bgr_fill_coverage_batch, "INPAINT") as
loops over lists, written independently of tests/_inpaint_ref.py so that the two can be held against each other.

Test infrastructure only: nothing of the product is used here.
"""
import numpy as np


def inpaint(img, mask):
    H, W = len(mask), len(mask[0])
    val = [[[int(img[y][x][c]) if mask[y][x] else None for c in range(3)] for x in range(W)] for y in range(H)]
    keep = [[bool(mask[y][x]) for x in range(W)] for y in range(H)]
    pyramid = [(W, H, val, keep)]
    # push
    while not (W == 1 and H == 1):
        W1, H1 = (W + 1) >> 1, (H + 1) >> 1
        nval = [[None] * W1 for _ in range(H1)]
        nkeep = [[False] * W1 for _ in range(H1)]
        for Y in range(H1):
            for X in range(W1):
                kids = [(2 * X + i, 2 * Y + j) for j in (0, 1) for i in (0, 1)]
                kids = [(x, y) for x, y in kids if x < W and y < H and keep[y][x]]
                n = len(kids)
                if n == 0:
                    continue
                nkeep[Y][X] = True
                nval[Y][X] = [(2 * sum(val[y][x][c] for x, y in kids) + n) // (2 * n) for c in range(3)]
        W, H, val, keep = W1, H1, nval, nkeep
        pyramid.append((W, H, val, keep))
    if not pyramid[-1][3][0][0]:
        return np.array(img, copy=True)
    # pull
    for lvl in range(len(pyramid) - 2, -1, -1):
        W, H, val, keep = pyramid[lvl]
        W1, H1, up, _ = pyramid[lvl + 1]
        for y in range(H):
            py = y >> 1
            qy = min(max(py + (1 if y & 1 else -1), 0), H1 - 1)
            for x in range(W):
                if keep[y][x]:
                    continue
                px = x >> 1
                qx = min(max(px + (1 if x & 1 else -1), 0), W1 - 1)
                val[y][x] = [(9 * up[py][px][c] + 3 * up[py][qx][c] + 3 * up[qy][px][c] + up[qy][qx][c] + 8) >> 4 for c in range(3)]
        # (the level's mask is left as it was: only `val` is complete now, which is all the level below reads)
    out = np.array(img, copy=True)
    _, _, val, _ = pyramid[0]
    for y in range(len(mask)):
        for x in range(len(mask[0])):
            if not mask[y][x]:
                out[y, x] = val[y][x]
    return out
