"""GPU: the persistent and grid-stride kernels past their first round, on REAL values.

The "rounds-" cases of test_gpu_exact.py give a workgroup of conv3x3_tap_stream_kernel, stem_v3_kernel and first_pool_mfma*_kernel its second
and third tile, and the grid-stride kernels of aux.hip their second round, bit for bit -- but on integer data: hidden layers non-negative,
operands at most 8.  Here the same graphs run

- on synth.synthetic_input / synth.darknet_stream against the oracle, through test_gpu_ops.check_graph at that module's tolerance (every
  layer a fusion does not swallow read back; the stem does not plan with keep_all and is read through the layers behind it);
- on uint8 input: forward_u8 is bit-identical to forward fed float32(u / 255.) where the kernel that reads the input is past its cap (the
  uint8 twins of the stem, of the three first-layer MFMA kernels and of prep_kernel), in one pass and as two parts on two streams;
- and decode_kernel past its 524 288 rows through yolo_decode_nms against oracle/decode_ref.py.

No tolerance of its own anywhere.  Which cap a case is about and how many rounds it claims is in the tables (test_gpu_exact.ROUNDS, U8_CASES,
DECODE); tests/test_rounds_cpu.py holds them against yolo_launch_caps without a GPU.  A failed comparison names the tile of the first
element beyond the tolerance and whether its workgroup was past its first tile.
"""
import zlib

import numpy as np
import pytest

import test_gpu_exact as T
from helpers import match_boxes
from oracle import cases, decode_ref
from tensorflow_yolo_amd.net import engine, synth

pytestmark = pytest.mark.gpu

ROUNDS_IDS = [cid for cid in T.IDS if cid in T.ROUNDS]

# layers read back with keep_all where that leaves the kernel the case is about in place: a fused residual / pool is unfused by keep_all
# (another launch), and the stem does not plan with it
FALLBACK_READ = (3, 5, 6, 8, 9)


def read_layers(c, variant):
    name = c["graph"][0]
    if name == "g_fallback":
        return FALLBACK_READ
    if name == "g_probe" and variant == "pool":
        return (1,)
    return ()


def real_input(c, variant):
    g = T.build_graph(c, variant)
    h, w, ch = g[0].out.hwc
    x = synth.synthetic_input(c["B"], h, w, ch, seed=zlib.crc32(c["id"].encode()) % 1000)
    return g, (x if ch == 3 else x * 2 - 1)             # (3 channels: an image in [0, 1); else both signs)


def first_beyond(rounds, batch):
    """check_graph's `where`: the tile of the first element whose error is above the tolerance (of the tensor's magnitude, as rel_err)"""
    def where(key, got, want, tol):
        err = np.abs(got.astype(np.float64) - want)
        lim = tol * max(1e-6, float(np.max(np.abs(want))))
        idx = np.argwhere(~(err <= lim))
        # (every tensor compared here is on the output grid of the kernel the case is about: read_layers)
        return "  %s: %d elements beyond %.3g, the first at (n, y, x, c) = %s in %s" % (
            key, len(idx), lim, tuple(int(v) for v in idx[0]), T.where_in_rounds(rounds, idx[0], got.shape, batch))
    return where


@pytest.mark.parametrize("cid", ROUNDS_IDS)
def test_real_values_against_the_oracle(cid):
    from test_gpu_ops import check_graph
    c = T.CASES[T.IDS.index(cid)]
    for variant in c["variants"]:
        g, x = real_input(c, variant)
        read = read_layers(c, variant)
        kw = dict(c["kw"])
        eng = check_graph(g, x, c["dtype"], seed=zlib.crc32(cid.encode()) % 997, read=read, max_batch=kw.pop("max_batch", None),
                          where=first_beyond(T.ROUNDS[cid], c["B"]), **kw)
        names, text = T.kernel_text(eng, eng.kernel_infos())
        T.check_kernels(c, variant, eng, names, text)           # the kernel meant is the one that ran, with keep_all as well
        assert eng.num_streams == T.ROUNDS[cid]["parts"], (cid, eng.num_streams)


# ---- uint8 input past the caps ------------------------------------------------------------------------------------------------
# name: (exact case whose graph and dtype it takes, streams, symbol of the float32 kernel that reads the input, claim).  The three-round
# shapes; as two parts each part is still past its cap (stem: 546 tiles on 256 workgroups; first layer: 1125 tiles on 1024).  prep_kernel's
# case is past its cap in one pass only (538 240 pixels per part) and runs in one pass.
U8_CASES = {}
for _cid, _sym in [("rounds-stem-3-32-64-32-6x224x416", "yolo::stem_v3_kernel("), ("rounds-firstpool-10x240x464-32-fp16", "yolo::first_pool_mfma_kernel("),
                   ("rounds-firstpool-10x240x464-32-fp32", "first_pool_mfma_f32_kernel<2>("), ("rounds-firstpool-10x240x464-16-fp32", "first_pool_mfma_f32_kernel<1>("),
                   ("rounds-prep-5x464x464x8-fp16", "prep_kernel<false>("), ("rounds-prep-5x464x464x8-fp32", "prep_kernel<true>(")]:
    for _st in (1, 2):
        if _st == 1 or "prep" not in _cid:
            U8_CASES["%s-u8-streams%d" % (_cid[len("rounds-"):], _st)] = (_cid, _st, _sym, "three" if _st == 1 and "prep" not in _cid else "two")


def u8_plan_args(name):
    """(graph, dtype, engine keywords) of a uint8 case"""
    cid, streams, _, _ = U8_CASES[name]
    c = T.CASES[T.IDS.index(cid)]
    return T.build_graph(c, c["variants"][0]), c["dtype"], dict(max_batch=c["B"], keep_all=c["keep_all"], streams=streams), c


@pytest.mark.parametrize("name", sorted(U8_CASES))
def test_forward_u8_is_bit_identical_past_the_caps(name):
    """forward_u8(U) == forward(float32(U / 255.)) bit for bit; image 0 all 0, image 1 all 255, image 2 covering 0..255, the rest random bytes
    (the last images are the ones the later rounds compute)"""
    g, dtype, kw, c = u8_plan_args(name)
    eng = engine.HipNetwork(g, dtype=dtype, **kw)
    eng.load_weights(synth.darknet_stream(g, seed=11))
    text = " ".join(k.symbol.decode() for k in eng.kernel_infos())
    assert U8_CASES[name][2] in text and eng.num_streams == U8_CASES[name][1], (name, eng.num_streams, text)
    h, w, ch = eng.input_hwc
    u = np.random.default_rng(zlib.crc32(name.encode())).integers(0, 256, size=(c["B"], h, w, ch), dtype=np.uint8)
    u[0], u[1] = 0, 255
    u[2] = (np.arange(h * w * ch) % 256).astype(np.uint8).reshape(h, w, ch)
    want = eng.forward((u.astype(np.float64) / 255.).astype(np.float32)).cpu().numpy()
    got = eng.forward_u8(u).cpu().numpy()
    assert eng.u8_calls == 1 and np.isfinite(want).all() and np.abs(want).max() > 0
    if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        idx = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        rounds = dict(T.ROUNDS[U8_CASES[name][0]], parts=U8_CASES[name][1])
        raise AssertionError("%s: %d of %d elements differ, the first at (n, y, x, c) = %s in %s" % (
            name, len(idx), got.size, tuple(int(v) for v in idx[0]), T.where_in_rounds(rounds, idx[0], got.shape, c["B"])))


# ---- decode_kernel past its rows ------------------------------------------------------------------------------------------------
# A YOLOv2 head of 64 x 64 cells, 8 anchors (YOLO_MAX_ANCHORS), 1 class, 17 images: 557 056 rows (13 MB of logits) on a grid that holds
# 524 288 -- every row of the LAST image is computed by a thread in its second round.  Seeded as oracle/cases.make_head seeds its heads.  One
# class: p = sigmoid(objectness), so the shift of the objectness logit sets the candidate count: P(N(-3, 1) >= 0) = 1.35e-3 of 32 768 rows
# = 44 expected per image, far from both 0 and the candidate capacity.
DECODE = dict(version=2, input_hw=(2048, 2048), batch=17, classes=1, seed=91, scale=1.0, obj_shift=-3.0, cls_boost=0.0, threshold=0.5, iou=0.3,
              anchors=cases.COCO_V2_ANCHORS + cases.VOC_TINY_ANCHORS[:6], ties=0, box_scale=0.1)
DECODE_CAND_CAPACITY = 4096


def decode_rows(c=DECODE):
    return c["batch"] * cases.head_rows(c)[0]


def test_decode_past_its_rows():
    c = DECODE
    head = cases.make_head(c)
    anchors = np.reshape(c["anchors"], [-1, 2])
    assert head.shape == (17, 64, 64, 8 * 6)
    cand = decode_ref.find_bounding_boxes_v2(head, c["threshold"], c["iou"], anchors, c["classes"], nms=False)
    counts = [len(b) for b in cand]
    assert all(1 <= n <= DECODE_CAND_CAPACITY for n in counts), counts         # from the reference alone, before the GPU is touched
    rows_per_image = cases.head_rows(c)[0]
    last = [(c["batch"] - 1) * rows_per_image + b.scan for b in cand[-1]]        # rows of the last image's candidates in the whole launch
    cap = _hip_caps()["decode_rows"]
    assert last and min(last) >= cap, (min(last), cap)
    want = decode_ref.find_bounding_boxes_v2(head, c["threshold"], c["iou"], anchors, c["classes"])
    assert any(len(w) < n for w, n in zip(want, counts)), "NMS suppresses nothing"
    hd = engine.head_desc_v2(64, 64, anchors, c["classes"])
    recs, status = engine.decode_nms(hd, head, c["threshold"], c["iou"], cand_capacity=DECODE_CAND_CAPACITY)
    assert not status.any()
    print("candidates per image", counts, "survivors", [len(r) for r in recs])
    for i in range(c["batch"]):
        try:
            match_boxes(recs[i], [b.astuple() for b in want[i]])
        except AssertionError as e:
            raise AssertionError("image %d (rows %d..%d; rows at or above %d are a thread's second round): %s" % (
                i, i * rows_per_image, (i + 1) * rows_per_image - 1, cap, e))


def _hip_caps():
    from tensorflow_yolo_amd import _hip
    return _hip.launch_caps()
