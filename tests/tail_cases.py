"""The case table of the tail-training tests (tests/test_train_tail_cpu.py checks the table itself against the library's plan;
tests/test_gpu_train_tail.py runs it).  Nothing here touches a device."""
import numpy as np

# (ld - cin, coff, image stride beyond positions_per_image * ld, elements the view starts behind the buffer's first):
# dense; a slice of a wider pixel with a gap between the images; ld, coff, the image stride and the start no multiple of a 16-byte chunk
VIEWS = ((0, 0, 0, 0), (8, 8, 24, 0), (5, 3, 7, 1))

# ---- yolo_conv1x1_dgrad --------------------------------------------------------------------------------------------------------------------
DGRAD_COUTS = (1, 30, 425)            # one product per sum; no multiple of the 16-cout stage; the YOLOv2 head: 26 whole stages and 9 couts
DGRAD_CINS = (8, 40, 136, 1024)       # below one row of 4 channels x 2 lane halves; a tile with 40 of 128 channels; one past a tile; eight tiles
# (batch, positions per image): one position; 17; no multiple of the 64-position tile and more than one tile, two images; three tiles
DGRAD_POSITIONS = ((1, 1), (1, 17), (2, 37), (3, 50))
DGRAD_TILE_POSITIONS = 64             # kDgradTilePos (train_tail_host.h); test_train_tail_cpu.py checks the table against it


def y_values(rng, n):
    """stored activations for the slope branch: +0, -0, negatives and positives, small integers and halves (exact in fp16)"""
    pool = np.array([0.0, -0.0, -1.0, 1.0, -0.5, 0.5, -8.0, 8.0, 3.0, -3.0])
    return pool[rng.randint(0, len(pool), size=n)]


# ---- small nets from layer lists ----------------------------------------------------------------------------------------------------------
def small_tail_network(anchors, class_names, is_training, scope="yolo", input_shape=(64, 64, 3), residual=False):
    """the start of tiny-YOLOv2 (16, 32, 64 with 2 x 2 / 2 pools), a 3 x 3 conv to 128 and a pool, then the tail: a 3 x 3 / batch norm /
    leaky block 128 -> 128 and the detection layer -- stride 16, small enough for a float64 loop over every weight of the tail.
    residual: the block's output is added to its input (the planner fuses the shortcut into the block): no tail to train"""
    from tensorflow_yolo_amd.net import layers as PL, v2
    net = v2._start(input_shape)
    for filters in (16, 32, 64, 128):
        net.append(PL.conv2d_bn_act(net[-1].out, filters, 3, stride=1))
        net.append(PL.max_pool2d(net[-1].out, 2, stride=2))
    before = net[-1]
    net.append(PL.conv2d_bn_act(net[-1].out, 128, 3, stride=1))
    if residual:
        net.append(PL.shortcut(net[-1].out, before.out))
    v2._head_conv(net, len(anchors), len(class_names), {})
    net.anchors, net.num_classes = np.reshape(np.asarray(anchors, dtype=np.float64), [-1, 2]), len(class_names)
    return net


# ---- yolo_conv3x3_wgrad --------------------------------------------------------------------------------------------------------------------
WGRAD_HW = ((1, 1), (1, 5), (5, 1), (3, 3), (5, 7), (13, 13))
WGRAD_BATCHES = (1, 2, 3)
WGRAD_CINS = (8, 40, 136)             # one 8-channel load; 40 of a tile's 64; three tiles, the last of 8 channels
WGRAD_COUTS = (1, 30, 64, 65, 136)    # one; below an MFMA tile; exactly a workgroup tile; one past it; three tiles
CHUNK_CASE = (13, 13, 2)              # the shape the chunk properties are asserted on (test_train_tail_cpu.py)


def wgrad_shapes():
    """(h, w, batch, cin, cout): every map size with every batch, the channel counts cycling so that each appears with each map size;
    and every cin x cout at 13 x 13, batch 2"""
    pairs = [(cin, cout) for cout in WGRAD_COUTS for cin in WGRAD_CINS]
    out, i = [], 0
    for h, w in WGRAD_HW:
        for b in WGRAD_BATCHES:
            cin, cout = pairs[(7 * i) % len(pairs)]
            out.append((h, w, b, cin, cout))
            i += 1
    out += [CHUNK_CASE + p for p in pairs if CHUNK_CASE + p not in out]
    return out


def wgrad_plan_shapes(plan):
    """(h, w, batch) sized from yolo_conv3x3_wgrad_plan (`plan`: (h, w, batch) -> its dict) and not hard-coded: one position short of a
    chunk, exactly one chunk, one past it, and two chunks and five positions; w the largest divisor of the count up to 13"""
    c = plan(1, 1, 1)["positions_per_chunk"]
    out = []
    for P, chunks in ((c - 1, 1), (c, 1), (c + 1, 2), (2 * c + 5, 3)):
        w = max(d for d in range(1, 14) if P % d == 0)
        out.append((P // w, w, 1, chunks))
    return out
