"""The whole-network plans of tests/test_gpu_poison.py (part b: a poisoned twin equals a zeroed twin bit for bit), as a table that needs no
GPU: tests/test_poison_cpu.py plans every row with engine.Plan and holds the features a row is in the table for against the plan's own
text, so a later planner change fails there instead of quietly turning the GPU tests into tests of something else.

Sizes are the smallest that keep each plan's structure (a 160-wide first map still takes the stem, the pooled first conv and the tap
tiles; 96 x 160 leaves a 3 x 5 map in front of the SPP block).  Every plan names its stream count: streams = 0 lets the engine time one
pass against two halves on the device and keep the faster, and two twins must not differ by the outcome of a measurement."""
import functools

import numpy as np

import spp_ref
from oracle import cases
from tensorflow_yolo_amd import YoloV2, YoloV2Tiny, YoloV3, YoloV3SPP, YoloV3Tiny
from tensorflow_yolo_amd.net import synth

NAMES80 = ["c%d" % i for i in range(80)]
# network -> (class, anchors, class names, input height and width)
NETS = {"v2": (YoloV2, cases.COCO_V2_ANCHORS, NAMES80, (160, 160)),
        "v2-tiny": (YoloV2Tiny, cases.VOC_TINY_ANCHORS, NAMES80[:20], (160, 160)),
        "v3": (YoloV3, cases.COCO_V3_ANCHORS, NAMES80, (160, 160)),
        "v3-spp": (YoloV3SPP, cases.COCO_V3_ANCHORS, NAMES80, (96, 160)),
        "v3-tiny": (YoloV3Tiny, spp_ref.TINY_V3_ANCHORS, NAMES80, (96, 160))}
MAX_BATCH = 3
BATCHES = (3, 2)        # the full batch, and one image fewer: the last image's slots stay poisoned beside the work

PLANS = {}              # id -> dict(net, dtype, keep_all, kw (engine options), batches)


def _plan(net, dtype, keep_all, streams=1, max_batch=MAX_BATCH, batches=BATCHES):
    pid = "%s-%s-%s%s" % (net, dtype, "keep_all" if keep_all else "plan", "-streams%d" % streams if streams > 1 else "")
    PLANS[pid] = dict(net=net, dtype=dtype, keep_all=keep_all, kw={"streams": streams, "max_batch": max_batch}, batches=batches)


for _net in ("v2", "v2-tiny", "v3", "v3-spp", "v3-tiny"):
    for _dt in ("fp16", "fp32"):
        for _keep in (True, False):
            _plan(_net, _dt, _keep)
for _keep in (True, False):
    _plan("v3", "mxfp8", _keep)
_plan("v3", "fp16", False, streams=2, max_batch=6, batches=(5,))      # two parts, each in its own arena; 5 = 3 + 2 images

# What a row is in the table for: substrings of the plan's kernel names + symbols + description (test_gpu_exact.kernel_text) that must
# be there.  ("streams": Plan.num_streams, held for every row.)
FEATURES = {
    "v3-fp16-plan": ("conv_stem<f16,3-32-64-32>", "computed by the conv in front of it", "fused: +shortcut", "fused: upsample x2", "concat slice"),
    "v3-fp16-plan-streams2": ("conv_stem<f16,3-32-64-32>",),
    "v3-fp32-plan": ("fused: +shortcut", "fused: upsample x2"),
    "v3-mxfp8-plan": ("conv_mx", "conv_stem<f16,3-32-64-32>"),
    "v3-mxfp8-keep_all": ("conv_mx",),
    "v2-tiny-fp16-plan": ("conv_first_pool", "pool<"),
    "v2-tiny-fp32-plan": ("conv_first_pool", "pool<"),
    "v2-fp16-plan": ("conv_first_pool", "tap9,2d", "fused: reorg x2"),
    "v2-fp32-plan": ("conv_first_pool", "tap9,2d", "fused: reorg x2"),
    "v3-spp-fp16-plan": ("spp_pool<f16,5-9-13>", "conv_stem<f16,3-32-64-32>"),
    "v3-spp-fp16-keep_all": ("spp_pool<f16,5-9-13>",),
    "v3-spp-fp32-plan": ("pool_same",),
    "v3-tiny-fp16-plan": ("conv_first_pool", "pool<"),
    "v3-tiny-fp32-plan": ("conv_first_pool", "pool<"),
}


def create_network(net):
    cls, anchors, names, hw = NETS[net]
    return cls.create_network(np.reshape(anchors, [-1, 2]), names, False, input_shape=hw + (3,))


@functools.lru_cache(maxsize=2)
def weights_of(net, seed=41):
    """the synthetic Darknet stream of a network (objectness bias 0: calibrate_model re-centres it where a test detects); shared among
    the tests of one network, read-only (62 M floats for YOLOv3: the two networks last used stay)"""
    cls, anchors, names, hw = NETS[net]
    w = synth.darknet_stream(create_network(net), seed=seed, num_classes=len(names), head_gain=synth.HEAD_DEFAULTS[cls.version][0], obj_bias=0.0)
    w.setflags(write=False)
    return w


def build_model(pid, weights=None, **more):
    """a Yolo model with the engine of plan `pid`; weights = None: nothing loaded yet (the poisoned twin fills the weight buffer first)"""
    p = PLANS[pid]
    cls, anchors, names, hw = NETS[p["net"]]
    m = cls()
    kw = dict(p["kw"], **more)
    m.build(anchors, names, hw + (3,), dtype=p["dtype"], max_batch=kw.pop("max_batch"), weights=weights, keep_all=p["keep_all"], **kw)
    return m


def plan_only(pid):
    """engine.Plan of a row (no GPU)"""
    from tensorflow_yolo_amd.net import engine
    p = PLANS[pid]
    kw = dict(p["kw"])
    return engine.Plan(create_network(p["net"]), dtype=p["dtype"], max_batch=kw.pop("max_batch"), keep_all=p["keep_all"], **kw)
