"""CPU: each of the planner's seven launch-fusion rules (csrc/plan.cpp: Planner::try_*) fires on a net it was
written for, and its opt-out variable -- read at every yolo_net_create, so set here between two plans of one process -- keeps it from
firing without changing what the net computes: same weight stream, same output, same FLOPs.  No compute calls."""
import numpy as np
import pytest

from oracle import cases
from tensorflow_yolo_amd.net import engine, v2, v3

NAMES80 = ["c%d" % i for i in range(80)]
NETS = {
    "v3-416": lambda: v3.create_network(np.reshape(cases.COCO_V3_ANCHORS, [-1, 2]), NAMES80, False, input_shape=(416, 416, 3)),
    "v3spp-416": lambda: v3.create_spp_network(np.reshape(cases.COCO_V3_ANCHORS, [-1, 2]), NAMES80, False, input_shape=(416, 416, 3)),
    "v2-416": lambda: v2.create_full_network(np.reshape(cases.COCO_V2_ANCHORS, [-1, 2]), NAMES80, False),
}
# (variable, net, the note the rule leaves in the plan)
RULES = [
    ("YOLO_NO_FIRST_DIRECT", "v2-416", "direct conv on the float32 input (no cast/pad pass)"),
    ("YOLO_NO_STEM", "v3-416", "fused with the first layer (stem.hip)"),
    ("YOLO_NO_STEM3", "v3-416", "computed inside the stem kernel (no launch)"),
    ("YOLO_NO_FUSE2", "v3-416", "computed by the conv in front of it"),
    ("YOLO_NO_FIRST_POOL", "v2-416", "+ fused 2x2/2 max-pool (layer 2)"),
    ("YOLO_NO_CONV_POOL", "v2-416", "+ fused 2x2/2 max-pool (layer 4)"),
    ("YOLO_NO_SPP_FUSE", "v3spp-416", "fused SPP block"),
]
_nets = {}


@pytest.mark.parametrize("var,net,note", RULES, ids=[r[0] for r in RULES])
def test_switch_is_read_at_every_plan(monkeypatch, var, net, note):
    if net not in _nets:
        _nets[net] = NETS[net]()
    for v, _, _ in RULES:
        monkeypatch.delenv(v, raising=False)
    on = engine.Plan(_nets[net], dtype="fp16", max_batch=2)
    assert note in on.describe()
    monkeypatch.setenv(var, "1")
    off = engine.Plan(_nets[net], dtype="fp16", max_batch=2)
    assert note not in off.describe()
    monkeypatch.delenv(var)
    again = engine.Plan(_nets[net], dtype="fp16", max_batch=2)
    assert again.describe() == on.describe()
    for p in (off, again):
        assert (p.weight_count, p.output_count, p.flops_per_image) == (on.weight_count, on.output_count, on.flops_per_image)
