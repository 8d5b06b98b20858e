"""CPU: what the six host-only training entries answer for every shipped network, pinned value by value -- every field of
yolo_net_head_input, yolo_net_head_train_layout, yolo_net_tail_inputs, yolo_net_tail_train_layout, yolo_net_head_inputs_v3 and
yolo_net_head_train_v3_layout, or the status and the whole yolo_last_error() text where an entry refuses the net, and the three
*_train_bytes values.  The other CPU tests bound these numbers (total_bytes >= ...); this one holds them still, so that a change of the
host code behind them (csrc/train_api.cpp) shows as a changed offset or a changed message.

The record, tests/golden/train_layouts.json, was written by the library of the commit BEFORE the training entries moved out of api.cpp
(YOLO_HIP_LIB pointing at that build; `python tests/test_train_layouts_cpu.py` calls record()).  Rewrite it only after a deliberate
change of a layout or a message."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from helpers import GOLDEN
import spp_ref
from oracle import cases
from tensorflow_yolo_amd import _hip
from tensorflow_yolo_amd.net import engine, v2, v3

LAYOUTS_JSON = os.path.join(GOLDEN, "train_layouts.json")
NAMES3 = ["a", "b", "c"]
HW = (96, 160)          # not square; a 3 x 5 grid at stride 32
NETS = {"v2": (v2.create_full_network, cases.COCO_V2_ANCHORS), "tiny-v2": (v2.create_tiny_network, cases.VOC_TINY_ANCHORS),
        "v3": (v3.create_network, cases.COCO_V3_ANCHORS), "v3-tiny": (v3.create_tiny_network, spp_ref.TINY_V3_ANCHORS),
        "v3-spp": (v3.create_spp_network, cases.COCO_V3_ANCHORS)}
DTYPES = ("fp16", "fp32", "mxfp8")
BATCHES = (1, 2, 3, 8)      # 1 and 2: where the bounds of a "largest split of any batch up to max_batch" loop show
# every (net, dtype, max_batch) on one stream, and each net once as two stream parts (the `stream parts` refusal)
GRID = [(n, d, b, 1) for n in sorted(NETS) for d in DTYPES for b in BATCHES] + [(n, "fp16", 8, 2) for n in sorted(NETS)]


def key_of(net, dtype, batch, streams):
    return "%s %s b%d streams%d" % (net, dtype, batch, streams)


def fields(s):
    """every field of a ctypes structure as JSON values (arrays as lists)"""
    return {n: (list(getattr(s, n)) if hasattr(getattr(s, n), "__len__") else getattr(s, n)) for n, _ in s._fields_}


def answer(lib, rc, *structs):
    if rc:
        return {"status": rc, "error": lib.yolo_last_error().decode()}
    return {"status": 0, "fields": [fields(s) for s in structs]}


def plan_of(net, dtype, batch, streams):
    make, anchors = NETS[net]
    try:
        p = engine.Plan(make(np.reshape(anchors, [-1, 2]), NAMES3, False, input_shape=HW + (3,)), dtype=dtype, max_batch=batch, streams=streams)
    except _hip.YoloHipError:       # the net has no such plan
        return None
    if net in ("v2", "tiny-v2"):
        p.set_head(engine.head_desc_v2(HW[0] // 32, HW[1] // 32, anchors, len(NAMES3)))
    return p


def answers(net, dtype, batch, streams):
    """what the entries say of one plan: {entry: {"status": 0, "fields": [...]} | {"status": rc, "error": text} | bytes}"""
    p = plan_of(net, dtype, batch, streams)
    if p is None:
        return None
    lib, h, out = p.lib, p.handle, {}
    v, b = _hip.TensorView(), _hip.TensorView()
    out["yolo_net_head_input"] = answer(lib, lib.yolo_net_head_input(h, C.byref(v)), v)
    lay = _hip.HeadTrainLayout()
    out["yolo_net_head_train_layout"] = answer(lib, lib.yolo_net_head_train_layout(h, C.byref(lay)), lay)
    out["yolo_net_tail_inputs"] = answer(lib, lib.yolo_net_tail_inputs(h, C.byref(b), C.byref(v)), b, v)
    tail = _hip.TailTrainLayout()
    out["yolo_net_tail_train_layout"] = answer(lib, lib.yolo_net_tail_train_layout(h, C.byref(tail)), tail)
    views, n = (_hip.TensorView * _hip.MAX_SCALES)(), C.c_int32(0)
    out["yolo_net_head_inputs_v3"] = answer(lib, lib.yolo_net_head_inputs_v3(h, views, C.byref(n)), *[views[s] for s in range(n.value)])
    lay3 = _hip.HeadTrainV3Layout()
    out["yolo_net_head_train_v3_layout"] = answer(lib, lib.yolo_net_head_train_v3_layout(h, C.byref(lay3)), lay3)
    for name in ("yolo_net_head_train_bytes", "yolo_net_tail_train_bytes", "yolo_net_head_train_v3_bytes"):
        out[name] = int(getattr(lib, name)(h))
    p.close()
    return out


def record():
    rec = {key_of(*g): answers(*g) for g in GRID}
    with open(LAYOUTS_JSON, "w") as f:
        json.dump(rec, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("%d plans (%d without a plan of that dtype) recorded in %s (%d bytes) from %s"
          % (len(rec), sum(v is None for v in rec.values()), LAYOUTS_JSON, os.path.getsize(LAYOUTS_JSON), _hip.LIB_PATH))


@pytest.fixture(scope="module")
def recorded():
    with open(LAYOUTS_JSON) as f:
        return json.load(f)


def test_the_record_covers_the_grid_and_every_kind_of_answer(recorded):
    assert sorted(recorded) == sorted(key_of(*g) for g in GRID)
    have = [v for v in recorded.values() if v is not None]
    assert len(have) >= 2 * len(BATCHES) * len(NETS) + len(NETS)          # fp16 and fp32 plans exist for every net
    for entry in ("yolo_net_head_input", "yolo_net_head_train_layout", "yolo_net_tail_inputs", "yolo_net_tail_train_layout",
                  "yolo_net_head_inputs_v3", "yolo_net_head_train_v3_layout"):
        assert {v[entry]["status"] == 0 for v in have} == {True, False}, entry       # each entry both answers and refuses somewhere
    for name in ("yolo_net_head_train_bytes", "yolo_net_tail_train_bytes", "yolo_net_head_train_v3_bytes"):
        assert any(v[name] > 0 for v in have) and any(v[name] == 0 for v in have), name
    for n in NETS:          # two stream parts: the entries of the net's own kind refuse with YOLO_ERR_STATE
        v = recorded[key_of(n, "fp16", 8, 2)]
        assert any(v[e]["status"] == 5 and "stream parts" in v[e]["error"] for e in v if not e.endswith("_bytes")), n


@pytest.mark.parametrize("net", sorted(NETS))
def test_layouts_views_and_refusals_equal_the_record(recorded, net):
    for g in GRID:
        if g[0] != net:
            continue
        want, got = recorded[key_of(*g)], answers(*g)
        if want is None:
            assert got is None, key_of(*g)
            continue
        assert got is not None and sorted(got) == sorted(want), key_of(*g)
        for entry in sorted(want):
            if entry.endswith("_bytes"):
                assert got[entry] == want[entry], (key_of(*g), entry)
                continue
            assert got[entry]["status"] == want[entry]["status"], (key_of(*g), entry, got[entry])
            if want[entry]["status"]:
                assert got[entry]["error"] == want[entry]["error"], (key_of(*g), entry)       # message by message
                continue
            assert len(got[entry]["fields"]) == len(want[entry]["fields"]), (key_of(*g), entry)
            for s, (a, b) in enumerate(zip(got[entry]["fields"], want[entry]["fields"])):
                assert sorted(a) == sorted(b), (key_of(*g), entry, s)
                for name in sorted(b):                                                       # field by field
                    assert a[name] == b[name], (key_of(*g), entry, s, name, a[name], b[name])


if __name__ == "__main__":      # rewrite the record (no GPU needed)
    record()
