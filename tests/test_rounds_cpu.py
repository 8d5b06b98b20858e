"""CPU: every "past the first round" case is past the first round -- by the library's own numbers.

The rounds cases of test_gpu_exact.py and test_gpu_rounds.py are sized from the launch caps of five kernel families (how many workgroups a
persistent kernel launches at most, how many threads a grid-stride kernel).  The caps are read from the library (yolo_launch_caps); the
work of a case is counted from its shape (tiles of 16 x 16 positions for conv3x3_tap_stream_kernel, of 16 x 32 input pixels for stem_v3_kernel
and first_pool_mfma*_kernel, elements / pixels / rows for the grid-stride kernels) and, where the plan reports the kernel's output map, from the
plan as well; a batch split over n streams runs n parts on cap / n workgroups each.  Each case claims a round count -- "control": one,
exactly filling the grid; "one-more": cap + 1 items, ONE workgroup gets a second tile; "three": at least three; "two": at least two -- and
the plan of each names the kernel it is about.  A later change of a cap turns these red; without them the GPU cases would quietly go back
to testing one round.
"""
import ctypes as C

import pytest

import test_gpu_exact as T
import test_gpu_rounds as R
from tensorflow_yolo_amd import _hip
from tensorflow_yolo_amd.net import engine

CAPS = ("tap_stream_workgroups", "stem_workgroups", "first_mfma_workgroups", "aux_work_items", "decode_rows")
# what the cases were sized for: launch_conv_tap (256 CUs x 2 resident workgroups), launch_stem, launch_first, aux.hip grid_for (4096 blocks
# of 256), launch_decode (2048 blocks of 256)
SIZED_FOR = {"tap_stream_workgroups": 512, "stem_workgroups": 512, "first_mfma_workgroups": 1024, "aux_work_items": 1048576, "decode_rows": 524288}


def rounds_of(work, cap, parts=1):
    return T._cdiv(work, cap // parts)


def check_claim(what, claim, work, cap, parts=1):
    n = rounds_of(work, cap, parts)
    per_part = cap // parts
    if claim == "control":
        assert n == 1 and work == per_part, "%s: %d items on %d: not exactly one full round" % (what, work, per_part)
    elif claim == "one-more":
        assert work == per_part + 1, "%s: %d items on %d: not cap + 1" % (what, work, per_part)
    elif claim == "three":
        assert n >= 3, "%s: %d items on %d: %d round(s), not three" % (what, work, per_part, n)
    else:
        assert claim == "two" and n >= 2, "%s: %d items on %d: %d round(s), not two" % (what, work, per_part, n)
    return n


def test_the_caps_are_what_the_cases_were_sized_for():
    caps = _hip.launch_caps()
    assert tuple(caps) == CAPS and C.sizeof(_hip.LaunchCaps) == 20
    assert caps == SIZED_FOR, "a launch cap changed: resize the rounds cases of test_gpu_exact.py / test_gpu_rounds.py (%r)" % (caps,)
    assert _hip.lib().yolo_launch_caps(None) != 0 and b"null" in _hip.lib().yolo_last_error()


def _work_from_shape(c, r):
    """the work count of a rounds case (r: its ROUNDS entry) from its graph arguments alone, per part"""
    name, a = c["graph"]
    B = T._cdiv(c["B"], r["parts"])
    if r["cap"] == "tap_stream_workgroups":
        return B * T._cdiv(a[0], 16) * T._cdiv(a[1], 16)
    if r["cap"] in ("stem_workgroups", "first_mfma_workgroups"):
        return B * T._cdiv(a[0], 16) * T._cdiv(a[1], 32)
    if name == "g_fallback":            # the smallest eltwise launch of the graph: the upsample, counted in elements of its INPUT (the 2x2/2-pooled 32-channel map)
        return B * (a[0] // 2) * (a[1] // 2) * 32
    return B * a[0] * a[1]              # prep: pixels


def _kernel_of(p, sym):
    for k in range(p.num_kernels):
        ki = _hip.KernelInfo()
        _hip.check(p.lib.yolo_net_kernel_info(p.handle, k, C.byref(ki)), "yolo_net_kernel_info")
        if sym in ki.symbol.decode():
            return ki
    return None


@pytest.mark.parametrize("cid", R.ROUNDS_IDS)
def test_exact_and_operator_cases_run_the_rounds_they_claim(cid):
    c = T.CASES[T.IDS.index(cid)]
    r = T.ROUNDS[cid]
    cap = _hip.launch_caps()[r["cap"]]
    work = _work_from_shape(c, r)
    assert work == r["work"], (cid, work, r["work"])
    n = check_claim(cid, r["claim"], work, cap, r["parts"])
    for variant in c["variants"]:
        p, names, text = T.plan_of(c, variant)
        T.check_kernels(c, variant, p, names, text)             # names its kernel symbol (c["expect"]) -- on the plan the GPU test runs
        assert p.num_streams == r["parts"], (cid, p.num_streams)
        if r["tile"] is not None:       # the same count from the plan: the kernel's output map in tiles
            sym = {"tap_stream_workgroups": T.TAP_STREAM_SYM, "stem_workgroups": "stem_v3_kernel(", "first_mfma_workgroups": "first_pool_mfma"}[r["cap"]]
            ki = _kernel_of(p, sym)
            assert ki is not None, (cid, sym, names)
            th, tw = (16, 32) if r["cap"] == "first_mfma_workgroups" else r["tile"]       # (the plan reports the first conv's map in front of its fused pool)
            assert T._cdiv(c["B"], r["parts"]) * T._cdiv(ki.out_h, th) * T._cdiv(ki.out_w, tw) == work, (cid, ki.out_h, ki.out_w, work)
        # the operator test's plan (layers read back with keep_all) runs the same kernels
        read = R.read_layers(c, variant)
        if read and not c["keep_all"]:
            kw = dict(c["kw"])
            pk = engine.Plan(T.build_graph(c, variant), dtype=c["dtype"], max_batch=kw.pop("max_batch", c["B"]), keep_all=True, **kw)
            infos = [T._info(pk, k, C, _hip) for k in range(pk.num_kernels)]
            T.check_kernels(c, variant, pk, *T.kernel_text(pk, infos))
    print("%s: %d items on %d x %d: %d rounds (%s)" % (cid, work, r["parts"], cap // r["parts"], n, r["claim"]))


@pytest.mark.parametrize("name", sorted(R.U8_CASES))
def test_uint8_cases_run_the_rounds_they_claim(name):
    cid, streams, sym, claim = R.U8_CASES[name]
    g, dtype, kw, c = R.u8_plan_args(name)
    r = dict(T.ROUNDS[cid], parts=streams)              # (two streams: half the batch per part)
    check_claim(name, claim, _work_from_shape(c, r), _hip.launch_caps()[r["cap"]], streams)
    p = engine.Plan(g, dtype=dtype, **kw)
    assert p.num_streams == streams and _kernel_of(p, sym) is not None, (name, p.num_streams, p.describe())


def test_decode_case_runs_a_second_round():
    cap = _hip.launch_caps()["decode_rows"]
    c = R.DECODE
    rows = R.decode_rows()
    assert rows == 17 * 64 * 64 * 8 and len(c["anchors"]) // 2 == _hip.MAX_ANCHORS
    check_claim("decode", "two", rows, cap)
    assert (c["batch"] - 1) * (rows // c["batch"]) >= cap           # every row of the last image is a second-round row


def _xcd_remap(bid, n_blocks):
    """conv_common.h: xcd_remap"""
    q, r, x, y = n_blocks >> 3, n_blocks & 7, bid & 7, bid >> 3
    return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + y


def test_the_failure_report_names_tile_and_round():
    """what a failed comparison prints (test_gpu_exact.where_in_rounds): the launch position of a stream-kernel tile inverts xcd_remap, and
    the one second-round tile of the cap + 1 case is reported as such"""
    for n in (512, 513, 546, 1089):
        assert [_xcd_remap(T._launch_position("tap_stream_workgroups", g, n), n) for g in range(n)] == list(range(n))
    r = T.ROUNDS["rounds-tap-3x304x144x32x64"]          # 513 tiles of 19 x 9 per image: position 512 computes tile xcd_remap(512, 513) = 64
    assert _xcd_remap(512, 513) == 64
    shape = (3, 304, 144, 64)
    second = [g for g in range(513) if "AT OR ABOVE" in T.where_in_rounds(r, ((g // 171), (g % 171) // 9 * 16, (g % 9) * 16, 0), shape, 3)]
    assert second == [64]
    text = T.where_in_rounds(r, (0, 7 * 16 + 3, 1 * 16 + 5, 9), shape, 3)
    assert "(image 0, tile row 7, tile column 1)" in text and "launch position 512" in text and "the 2. tile" in text, text
    # two parts on two streams: the cap and the tile count are per part (images 3-5 are the second part)
    r = T.ROUNDS["rounds-stem-3-32-64-32-6x224x416-streams2"]
    text = T.where_in_rounds(r, (5, 111, 207, 0), (6, 112, 208, 64), 6)
    assert "tile 545, launch position 545" in text and "cap of 256" in text and "the 3. tile" in text, text
    # a grid-stride kernel: the linear element against the cap
    r = T.ROUNDS["rounds-prep-5x464x464x8-fp16"]
    assert "below" in T.where_in_rounds(r, (0, 0, 0, 0), (5, 464, 464, 16), 5) and "AT OR ABOVE" in T.where_in_rounds(r, (4, 463, 463, 15), (5, 464, 464, 16), 5)
