"""CPU: the host-side buffer layouts, pinned against a record (tests/golden/host_layout.json).

The workspace of a plan -- every activation tensor of every arena, then the tail: head logits, candidates, candidate counters, NMS
scratch, objectness, split-K tickets + slabs -- is laid out by the planner and reported by yolo_net_workspace_regions; the scratch of the
standalone decode + NMS is sized by yolo_decode_scratch_bytes.  For the plans of PLANS the record holds the whole region table and the
workspace size, and for SCRATCH the scratch sizes; the comparison is exact equality.  test_tail_is_contiguous asserts from the table
alone that the tail regions follow each other without a gap and end at workspace_bytes.

The record is a statement about behaviour: it was taken from the library of the commit BEFORE the layouts got one description each,
and a refactor must leave it untouched.  `python tests/test_layout_cpu.py` rewrites it after a deliberate change (with YOLO_HIP_LIB
pointing at another build of the library -- tools/build_ref_lib.sh --, from that build).
"""
import ctypes as C
import json
import os

from helpers import GOLDEN
from test_dispatch_cpu import NETS
from tensorflow_yolo_amd import _hip
from tensorflow_yolo_amd.net import engine

LAYOUT_JSON = os.path.join(GOLDEN, "host_layout.json")
TAIL = ["head logits", "candidates", "candidate counters", "nms scratch", "objectness", "split-K tickets + slabs"]

PLANS = [
    ("v3-608/fp16/b32", "v3-608", dict(dtype="fp16", max_batch=32)),                    # by rule: two full arenas
    ("v3-608/fp16/b32/streams1", "v3-608", dict(dtype="fp16", max_batch=32, streams=1)),
    ("v3-608/fp16/b32/streams3", "v3-608", dict(dtype="fp16", max_batch=32, streams=3)),
    ("v3-416/fp16/b2/keep_all", "v3-416", dict(dtype="fp16", max_batch=2, keep_all=True)),
    ("v2-416/fp32/b1", "v2-416", dict(dtype="fp32", max_batch=1)),                      # split-K region present
    ("tinyv2voc-416/fp32/b64", "tinyv2voc-416", dict(dtype="fp32", max_batch=64)),
    ("v3spp-416/fp16/b8", "v3spp-416", dict(dtype="fp16", max_batch=8)),
    ("v3-416/fp16/b4/cand16384", "v3-416", dict(dtype="fp16", max_batch=4, cand_capacity=16384)),      # NMS scratch region non-empty
]
SCRATCH = [(b, cap) for b in (1, 3, 32) for cap in (0, 1, 4096, 4097, 65536)]


def record_all():
    plans = {}
    for key, net, kw in PLANS:
        p = engine.Plan(NETS[net](), **kw)
        plans[key] = dict(workspace_bytes=int(p.workspace_bytes), regions=[list(r) for r in p.workspace_regions()])
        p.close()
    lib = _hip.lib()
    head = _hip.HeadDesc()
    scratch = {"b%d/cap%d" % (b, cap): int(lib.yolo_decode_scratch_bytes(C.byref(head), b, cap)) for b, cap in SCRATCH}
    return dict(plans=plans, decode_scratch_bytes=scratch)


_got = []


def got():
    if not _got:
        _got.append(record_all())
    return _got[0]


def want():
    with open(LAYOUT_JSON) as f:
        return json.load(f)


def test_workspace_regions_match_the_record():
    g, w = got()["plans"], want()["plans"]
    assert sorted(g) == sorted(w)
    for key in sorted(g):
        assert g[key]["workspace_bytes"] == w[key]["workspace_bytes"], key
        assert len(g[key]["regions"]) == len(w[key]["regions"]), key
        for a, b in zip(g[key]["regions"], w[key]["regions"]):
            assert a == b, (key, a, b)


def test_decode_scratch_bytes_match_the_record():
    assert got()["decode_scratch_bytes"] == want()["decode_scratch_bytes"]


def test_the_record_covers_what_it_is_for():
    w = want()["plans"]
    names = lambda key: [r[0] for r in w[key]["regions"]]
    assert any("arena 1" in n for n in names("v3-608/fp16/b32")) and not any("arena 1" in n for n in names("v3-608/fp16/b32/streams1"))
    assert any("arena 2" in n for n in names("v3-608/fp16/b32/streams3"))
    assert TAIL[5] in names("v2-416/fp32/b1")
    nms = {key: [r for r in w[key]["regions"] if r[0] == "nms scratch"][0] for key in w}
    assert nms["v3-416/fp16/b4/cand16384"][2] > 0 and nms["v3-608/fp16/b32"][2] == 0


def test_tail_is_contiguous():
    """From the table alone: the tail regions stand in offset order behind every activation tensor, each begins where the one before
    it ends, holds what it uses, and the last one ends at workspace_bytes."""
    for key, rec in got()["plans"].items():
        regions = rec["regions"]
        tail = [r for r in regions if not r[0].startswith("tensor ")]
        assert [r[0] for r in tail] == TAIL[:len(tail)] and len(tail) >= 5, key
        assert regions[-len(tail):] == tail, key
        assert tail[0][1] >= max(r[1] + r[3] for r in regions if r[0].startswith("tensor ")), key
        for a, b in zip(tail, tail[1:]):
            assert a[1] + a[3] == b[1], (key, a, b)
        for r in tail:
            assert r[2] <= r[3], (key, r)
        assert tail[-1][1] + tail[-1][3] == rec["workspace_bytes"], key


if __name__ == "__main__":      # rewrite the record (no GPU needed)
    with open(LAYOUT_JSON, "w") as f:
        json.dump(record_all(), f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("%d plans, %d scratch sizes recorded in %s (%d bytes) from %s"
          % (len(PLANS), len(SCRATCH), LAYOUT_JSON, os.path.getsize(LAYOUT_JSON), _hip.LIB_PATH))
