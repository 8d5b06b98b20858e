"""The yardstick of the YOLOv3 head-training tests: NumPy restatements of the definition in include/yolo_hip.h ("The weight gradient of the
YOLOv3 head convs").

terms               which (row, element) of G the assign table does not declare a structural zero: element 4 of every row, every element
                    of a row whose entry names a truth
scale_operands      G_s [P_s, cout_s] and the term mask of one scale, gathered out of [B, R, 5 + C]
wgrad_exact         dW_s, db_s in int64 for integer operands (any order gives these values while every partial sum stays below 2^24);
                    what the table declares a structural zero is never looked at, whatever G holds there
wgrad_ref64         the same in float64 with the bound (T + 2) 2^-24 S |G| |X| per element, T = the number of terms of the element
slot_table          slot[n][j] = the row truth j of image n owns, or -1
make_table, integer_g, shape_cases
                    the hand-made tables and operands of the exact tests, and their shapes, sized from yolo_v3_head_wgrad_plan
heads_train_loop64  forward of the head convs, loss and gradient (tests/loss_v3_ref.py), weight gradient and Adam in float64 on fixed features
"""
import numpy as np

import loss_v3_ref
import train_ref

GRIDS3, GRIDS1, GRID_ONE = ((2, 3), (4, 6), (8, 12)), ((2, 3),), ((1, 1),)
# (ld - cin, coff): dense; a slice of a wider pixel (still 16-byte periodic: the vector loads); a slice no 16-byte load fits (element loads)
VIEWS = train_ref.VIEWS + ((5, 3),)
PATTERNS = ("none", "one", "full-image", "edges", "two-anchors")
MAX_GT = 8


def scales_of(grids, A):
    """-> (R, [(row0, h, w, A)] per scale)"""
    return loss_v3_ref.rows_of(grids, [[(1., 1.)] * A] * len(grids))


def terms(table, width, max_gt):
    """bool [B, R, width]: True where a term is formed"""
    table = np.asarray(table)
    m = np.zeros(table.shape + (width,), dtype=bool)
    m[..., 4] = True
    m[(table >= 0) & (table < max_gt)] = True
    return m


def scale_operands(G, mask, scale):
    """(G_s [B * h * w, A * width], mask_s alike) of scale = (row0, h, w, A): position p = n * h * w + cell, column a * width + k"""
    row0, h, w, A = scale
    B, _, width = G.shape
    cut = lambda v: v[:, row0:row0 + h * w * A].reshape(B * h * w, A * width)
    return cut(G), cut(mask)


def wgrad_exact(Xs, G, table, grids, A, max_gt):
    """Xs: per scale the integer operand [P_s, cin_s]; G [B, R, width] (integers wherever a term is formed) -> [(dW int64, db int64)]"""
    R, scales = scales_of(grids, A)
    mask = terms(table, G.shape[2], max_gt)
    out = []
    for X, sc in zip(Xs, scales):
        Gs, Ms = scale_operands(G, mask, sc)
        Gi = np.where(Ms, Gs, 0).astype(np.int64)
        Xi = np.asarray(X).astype(np.int64)
        assert np.array_equal(Xi, X) and np.array_equal(Gi, np.where(Ms, Gs, 0)), "the exact reference takes integers"
        out.append((Gi.T @ Xi, Gi.sum(axis=0)))
    return out


def wgrad_ref64(Xs, G, table, grids, A, max_gt):
    """-> [(dW, db, bound_dW, bound_db)] in float64; bound = (T + 2) 2^-24 S |G| |X| per element over its T terms (|X| = 1 for db)"""
    R, scales = scales_of(grids, A)
    mask = terms(table, G.shape[2], max_gt)
    out = []
    for X, sc in zip(Xs, scales):
        Gs, Ms = scale_operands(G, mask, sc)
        G64, X64 = np.where(Ms, Gs, 0).astype(np.float64), np.asarray(X, dtype=np.float64)
        k = (Ms.sum(axis=0) + 2) * 2.0 ** -24            # T per output row o
        out.append((G64.T @ X64, G64.sum(axis=0), k[:, None] * (np.abs(G64).T @ np.abs(X64)), k * np.abs(G64).sum(axis=0)))
    return out


def slot_table(table, max_gt):
    table = np.asarray(table)
    slot = np.full((table.shape[0], max_gt), -1, dtype=np.int32)
    for n, r in zip(*np.nonzero((table >= 0) & (table < max_gt))):
        assert slot[n, table[n, r]] == -1, "a truth owns at most one row"
        slot[n, table[n, r]] = r
    return slot


def make_table(pattern, grids, A, B, rng, max_gt=MAX_GT):
    """A hand-made assign table [B, R]: a tenth of the rows ignored (-2), then the winners of `pattern`:
    none          no winner
    one           one row of one image
    full-image    max_gt truths in the middle image, none in its neighbours
    edges         the first row of every scale in image 0 (row 0 is the first of the batch), the last row of every scale in the last image
                  (its last row is the last of the batch)
    two-anchors   anchors 0 and 1 of one cell of scale 0, and the same of the last scale, in one image"""
    R, scales = scales_of(grids, A)
    table = np.where(rng.uniform(size=(B, R)) < 0.1, -2, -1).astype(np.int32)
    if pattern == "one":
        table[rng.randint(B), rng.randint(R)] = rng.randint(max_gt)
    elif pattern == "full-image":
        table[B // 2, rng.choice(R, size=min(max_gt, R), replace=False)] = rng.permutation(max_gt)[:min(max_gt, R)]
    elif pattern == "edges":
        assert 2 * len(scales) <= max_gt
        truths = rng.permutation(max_gt)
        for s, (row0, h, w, na) in enumerate(scales):
            table[0, row0] = truths[s]
            table[B - 1, row0 + h * w * na - 1] = truths[len(scales) + s] if B == 1 else truths[s]
    elif pattern == "two-anchors":
        assert A >= 2
        for j, (row0, h, w, na) in enumerate((scales[0], scales[-1])[:len(scales)]):
            cell = rng.randint(h * w)
            table[B - 1, row0 + cell * na] = 2 * j + 1
            table[B - 1, row0 + cell * na + 1] = 2 * j
    else:
        assert pattern == "none"
    return table


def integer_g(table, width, rng, max_gt=MAX_GT, poison=False):
    """G [B, R, width] float32 consistent with the table: integers in -8 .. 8 where a term is formed, +0 at element 4 of an ignored row, and
    in every structural zero +0 -- or, poisoned, NaN"""
    G = rng.randint(-8, 9, size=table.shape + (width,)).astype(np.float32)
    G[table == -2, 4] = 0
    G[~terms(table, width, max_gt)] = np.nan if poison else 0
    return G


def shape_cases(plan):
    """The shapes of the exact tests as (name, grids, A, C, cins, batch).  plan(grids, A, C, cins, batch) -> the dict of
    yolo_v3_head_wgrad_plan: the batches around a chunk of the objectness part are computed from it, not hard-coded.  With 6 positions per
    image no batch gives exactly one chunk or one position more, so a 1 x 1 grid carries those two (and the case sized from the
    number of chunks the reduce kernel stages at a time)."""
    ppc = plan(GRID_ONE, 3, 1, (8,), 1)["positions_per_chunk"][0]
    six = -(-ppc // 6)          # images of 2 x 3 that reach past one chunk
    tile = plan(GRID_ONE, 3, 1, (8,), 1)["reduce_tile_chunks"]
    return (
        ("three-scales", GRIDS3, 3, 3, (1024, 136, 40), 3),
        ("two-anchors-one-class", GRIDS3, 2, 1, (8, 40, 136), 2),
        ("row-of-85", GRIDS3, 3, 80, (40, 8, 136), 2),
        ("one-scale-below-a-chunk", GRIDS1, 3, 80, (1024,), six - 1),
        ("one-scale-past-a-chunk", GRIDS1, 3, 3, (136,), six if six * 6 > ppc else six + 1),
        ("one-scale-several-chunks", GRIDS1, 2, 1, (40,), 3 * six + 1),
        ("one-position-short", GRID_ONE, 3, 3, (40,), ppc - 1),
        ("exactly-one-chunk", GRID_ONE, 3, 3, (8,), ppc),
        ("one-position-more", GRID_ONE, 3, 3, (136,), ppc + 1),
        ("three-chunks-and-one", GRID_ONE, 2, 1, (40,), 3 * ppc + 1),
        # one chunk more than the reduce kernel stages at a time; the winner kernel walks its slots in many passes
        ("past-a-reduce-tile", GRID_ONE, 3, 1, (8,), tile * ppc + 1),
    )


def expected_chunks(name, P, ppc, tile):
    """what the case's name promises of the objectness part of its (first) scale"""
    n = -(-P // ppc)
    return {"past-a-reduce-tile": n == tile + 1 and P == tile * ppc + 1, "one-scale-below-a-chunk": P < ppc, "one-scale-past-a-chunk": n == 2, "one-scale-several-chunks": n >= 3,
            "one-position-short": P == ppc - 1, "exactly-one-chunk": P == ppc, "one-position-more": P == ppc + 1 and n == 2,
            "three-chunks-and-one": n == 4 and P == 3 * ppc + 1}.get(name, True)


def heads_train_loop64(Xs, Ws, bs, grids, anchors, n_classes, gt, counts, lr, steps, ignore_thresh=0.7):
    """`steps` Adam steps of the head convs alone on the fixed features Xs[s] [B * h_s * w_s, cin_s] (float64) -> (losses before each
    update, Ws, bs).  The logits pass through float32 on their way into the loss yardstick, as the device's do."""
    Xs = [np.asarray(X, dtype=np.float64) for X in Xs]
    Ws, bs = [np.array(W, dtype=np.float64) for W in Ws], [np.array(b, dtype=np.float64) for b in bs]
    R, scales = loss_v3_ref.rows_of(grids, anchors)
    B = Xs[0].shape[0] // (scales[0][1] * scales[0][2])
    width = 5 + n_classes
    mom = [[np.zeros_like(v) for v in (W, W, b, b)] for W, b in zip(Ws, bs)]
    losses = []
    for t in range(1, steps + 1):
        logits = np.concatenate([(X @ W.T + b).reshape(B, -1, width) for X, W, b in zip(Xs, Ws, bs)], axis=1)
        r = loss_v3_ref.loss(logits, grids, anchors, n_classes, gt, counts, ignore_thresh, mode="float64")
        losses.append(r["totals"]["loss"])
        G = r["grad"].astype(np.float64)
        lr_t = float(lr) * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)
        for s, (row0, h, w, na) in enumerate(scales):
            Gs = G[:, row0:row0 + h * w * na].reshape(B * h * w, na * width)
            Ws[s], mom[s][0], mom[s][1] = train_ref.adam_ref64(Ws[s], mom[s][0], mom[s][1], Gs.T @ Xs[s], lr_t)
            bs[s], mom[s][2], mom[s][3] = train_ref.adam_ref64(bs[s], mom[s][2], mom[s][3], Gs.sum(axis=0), lr_t)
    return losses, Ws, bs
