"""The case table of the tests of the sparse data gradient of a YOLOv3 head conv and of the 3 x 3 weight gradient on wide maps
(tests/test_train_blocks_v3_cpu.py checks the table itself against the library's plans; tests/test_gpu_train_blocks_v3.py runs it).
Nothing here touches a device."""
import numpy as np

import train_v3_ref

MAX_GT = 8
GRIDS3, GRIDS2, GRIDS1 = ((1, 1), (3, 5), (13, 13)), ((3, 5), (13, 13)), ((13, 13),)
# the patterns of tests/train_v3_ref.py (none; one; max_gt truths in one image; the first row of every scale in image 0 and the last row
# of every scale in the last image; anchors 0 and 1 of one cell) and two more: every anchor of one position of every scale a winner; rows
# whose entry names no truth (>= max_gt) and that hold full rows of G all the same
PATTERNS = train_v3_ref.PATTERNS + ("all-anchors", "beyond-max-gt")

# (name, grids, A, C, scale, cin, batch): every cin with scale 0, a middle scale and the last scale of 1- to 3-scale heads (row0 != 0
# wherever scale > 0), A 2 / 3, C 1 / 3 / 80, batch 1 - 3.  cin: one thread a position; 5 threads a position (one thread of the
# workgroup idle); 17 threads a position; a full channel tile, two positions a round; two channel tiles, the second of 8 channels
DGRAD_CASES = (
    ("cin8-scale0-of-3", GRIDS3, 3, 3, 0, 8, 3),
    ("cin8-last-of-3", GRIDS3, 2, 1, 2, 8, 2),
    ("cin40-middle-of-3", GRIDS3, 3, 80, 1, 40, 3),
    ("cin40-only-scale", GRIDS1, 2, 3, 0, 40, 1),
    ("cin136-last-of-2", GRIDS2, 3, 3, 1, 136, 2),
    ("cin136-scale0-of-2", GRIDS2, 2, 80, 0, 136, 3),
    ("cin1024-last-of-3", GRIDS3, 3, 1, 2, 1024, 2),
    ("cin1024-middle-of-3", GRIDS3, 2, 3, 1, 1024, 1),
    ("cin1032-last-of-2", GRIDS2, 3, 1, 1, 1032, 1),
)
REAL_CASES = (("13x13x136", GRIDS2, 3, 80, 1, 136, 2), ("cin1024", GRIDS3, 3, 80, 2, 1024, 1))

# (ld - cin, coff, image stride beyond positions_per_image * ld, elements the view starts behind the buffer's first): as tests/tail_cases.py
VIEWS = ((0, 0, 0, 0), (8, 8, 24, 0), (5, 3, 7, 1))


def loop_case(plan):
    """the smallest batch of 13 x 13 positions at cin 1024 whose workgroups walk a second round -- sized from yolo_v3_head_dgrad_plan
    (`plan`: (grids, A, C, scale, cin, batch) -> its dict), not hard-coded"""
    one = plan(GRIDS1, 2, 1, 0, 1024, 1)
    batch = (one["positions_per_round"] * 2048) // 169 + 1
    while not plan(GRIDS1, 2, 1, 0, 1024, batch)["loops"]:
        batch += 1
    return ("cin1024-second-round", GRIDS1, 2, 1, 0, 1024, batch)


def y_values(rng, n):
    """stored activations for the slope branch: +0, -0, negatives and positives, small integers and halves (exact in fp16)"""
    pool = np.array([0.0, -0.0, -1.0, 1.0, -0.5, 0.5, -8.0, 8.0, 3.0, -3.0])
    return pool[rng.randint(0, len(pool), size=n)]


def make_table(pattern, grids, A, B, rng, scale=0, max_gt=MAX_GT):
    """the hand-made assign tables [B, R] of tests/train_v3_ref.py, and the two patterns added above (`scale` is served first: a truth
    owns one row of an image, and max_gt of them do not reach every anchor of three scales)"""
    if pattern in train_v3_ref.PATTERNS:
        return train_v3_ref.make_table(pattern, grids, A, B, rng, max_gt)
    R, scales = train_v3_ref.scales_of(grids, A)
    table = np.where(rng.uniform(size=(B, R)) < 0.1, -2, -1).astype(np.int32)
    truths = list(rng.permutation(max_gt))
    for row0, h, w, na in [scales[scale]] + [sc for s, sc in enumerate(scales) if s != scale]:
        cell = rng.randint(h * w)
        for a in range(na):
            if pattern == "all-anchors":
                if truths:
                    table[B - 1, row0 + cell * na + a] = truths.pop()
            else:
                assert pattern == "beyond-max-gt"
                table[rng.randint(B), row0 + cell * na + a] = (max_gt, max_gt + 5, 2 ** 30)[a % 3]
    return table


def integer_g(table, width, rng, max_gt=MAX_GT, poison=False):
    """train_v3_ref.integer_g, but a row whose entry is >= max_gt holds a full row of integers (or, poisoned, NaN) outside element 4: the
    table declares them structural zeros, so they must not be read"""
    G = train_v3_ref.integer_g(table, width, rng, max_gt, poison)
    if not poison:
        beyond = np.asarray(table) >= max_gt
        G[beyond] = rng.randint(1, 9, size=(int(beyond.sum()), width))
    return G


# ---- yolo_conv3x3_wgrad on wide maps ---------------------------------------------------------------------------------------------------------
# (h, w, batch, cin, cout): the widths of the YOLOv3 / YOLOv3-tiny head blocks and the widest map the kernel takes, every cin with every
# cout, batch 1 and 2
WIDE_WGRAD_SHAPES = ((3, 26, 2, 8, 8), (3, 26, 1, 64, 64), (2, 38, 1, 8, 64), (2, 38, 2, 64, 8), (2, 76, 2, 8, 8), (2, 76, 1, 64, 64),
                     (2, 80, 1, 64, 8), (2, 80, 2, 8, 64))
WIDE_WGRAD_REFUSED = (2, 81, 1, 8, 8)


# ---- the twenty steps of tests/test_gpu_train_blocks_v3.py and their float64 loop on the CPU (tests/test_train_blocks_v3_cpu.py) ----------------
TRAIN_NAMES = ["a", "b", "c"]
TRAIN_ANCHORS = [10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326]
TRAIN_HW, TRAIN_BATCH, TRAIN_STEPS = (64, 64), 3, 20
TRAIN_TRUTHS = [[(0.3, 0.4, 0.2, 0.5, 1), (0.8, 0.2, 0.3, 0.3, 2), (0.5, 0.5, 0.9, 0.9, 0)], [], [(0.6, 0.6, 0.1, 0.15, 0), (0.1, 0.9, 0.05, 0.08, 2)]]
TRAIN_WEIGHT_SEED, TRAIN_INPUT_SEED = 41, 44
# the rate at which the yardstick's float64 loop lowers the loss at every one of the twenty steps (asserted on the CPU)
TRAIN_LR = 1e-5


def train_loop_args(net, weights, X3s, head):
    """the arguments of blocks_v3_ref.blocks_train_loop in front of (gt, counts, lr, steps, storage): the blocks and head convs cut out of
    the stream `weights` of the layer list `net`, the grids and anchors of the engine's head description `head`"""
    import tail_ref
    from tensorflow_yolo_amd.net import train as ytrain
    heads, blocks = ytrain.head_convs_v3(net), ytrain.block_convs_v3(net)
    ws, bs = ytrain.split_heads(weights, heads)
    blks = []
    for (pos, c3, i3), b in zip(blocks, ytrain.split_blocks(weights, blocks)):
        blks.append((b[:c3], b[c3:2 * c3], b[2 * c3:3 * c3], b[3 * c3:4 * c3], tail_ref.stream_to_otc(b[4 * c3:], c3, i3)))
    grids = [(head.h[s], head.w[s]) for s in range(head.n_scales)]
    anchors = [[(head.anchors[s][2 * a], head.anchors[s][2 * a + 1]) for a in range(head.n_anchors[s])] for s in range(head.n_scales)]
    return X3s, blks, ws, bs, grids, anchors, head.n_classes
