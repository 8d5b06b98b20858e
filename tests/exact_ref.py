"""Integer reference for the exact-arithmetic tests (test_exact_cpu.py, test_gpu_exact.py).

On integer data every product and every partial sum of a conv is exactly representable in the fp32 accumulator, in ANY summation
order, as long as conv(|x|, |w|) + |bias| < 2^24.  The result then no longer depends on tile, K order, split-K or fusion, and a
kernel's output must equal this reference bit for bit -- including the single fp16 rounding of its store.

  make_case(L, batch, seed)       seeded integer input / kernels / biases / BN parameters for an oracle layer list
  forward_exact(L, case, dtype)   the reference: float64 NumPy convs (exact below 2^53), float32 leaky / residual, one fp16 rounding
  check_preconditions(L, case, dtype)   what makes the equality a theorem; asserted before anything touches the GPU

Nothing here calls the torch oracle or the library's kernels (check_preconditions calls the library's HOST quantizer for MX layers).
L is the oracle's layer-tuple list (helpers.to_oracle).
"""
import numpy as np

import helpers  # noqa: F401  (puts the repository root on sys.path, as for mx_ref)
from oracle import topology

LEAKY = np.float32(0.1)          # conv_common.h / forward_ref._LEAKY: ONE float32 multiply
F24 = float(1 << 24)
F16_MAX = 65504.0
CHAIN_MAX = 2048                 # integers up to 2048 are exact in fp16
MX_MAX = 14                      # integers up to 14 are exact in e4m3fn at every block scale the quantizer can pick (scaled amax <= 448)
BN_VAR = np.float32(1.0 - 1e-5)  # gamma / sqrt(var + 1e-5) = 1 + 6.8e-9 in float64: w * scale rounds back to the integer w (|w| <= 2048)


def _sources(op):
    if op[0] in ("conv", "maxpool", "reorg", "upsample", "yolo"):
        return [op[1]]
    if op[0] == "shortcut":
        return [op[1], op[2]]
    if op[0] in ("route", "detection"):
        return list(op[1])
    return []


def consumers(L):
    cons = {}
    for i, op in enumerate(L):
        for s in _sources(op):
            cons.setdefault(s, []).append(i)
    return cons


def storage_rules(L):
    """forward_ref.forward(storage="fp16"): a conv whose ONLY consumer is a shortcut is rounded after the add (fused epilogue); the
    last conv and a conv that feeds only a yolo layer stay float32 (head)."""
    cons = consumers(L)
    fused, head = set(), set()
    for i, op in enumerate(L):
        if op[0] != "conv":
            continue
        c = cons.get(i, [])
        if len(c) == 1 and L[c[0]][0] == "shortcut":
            fused.add(i)
        if i == len(L) - 1 or (len(c) == 1 and L[c[0]][0] == "yolo"):
            head.add(i)
    return fused, head


def feeds_conv(L):
    """layers whose values reach a LATER conv (through data movement and adds): their stored values must keep the chain exact"""
    cons = consumers(L)
    out = set()
    for i in reversed(range(len(L))):
        for c in cons.get(i, []):
            if L[c][0] == "conv" or c in out:
                out.add(i)
    return out


def mx_candidates(L):
    """superset of the convs an mxfp8 plan may run on the MX kernel (plan.cpp mx_eligible: 3x3 / 1, Cin a multiple of 128)"""
    S = topology.shapes(L)
    return {i for i, op in enumerate(L) if op[0] == "conv" and op[3] == 3 and op[4] == 1 and S[op[1]][2] % 128 == 0}


# ---- operators ----------------------------------------------------------------------------------------------------------------
def _pad(x, k, s):
    """net/layers.py:9-14 / TF SAME for odd k and stride 1: (k-1)//2 before, the rest after"""
    a = (k - 1) // 2
    b = k - 1 - a
    return np.pad(x, ((0, 0), (a, b), (a, b), (0, 0))) if k > 1 else x


def conv_int(x, w_oihw, k, s):
    """x NHWC, w [o][i][kh][kw], both integer valued float64 -> float64 NHWC; one matmul per tap (exact below 2^53 in any order)"""
    n, h, wd, c = x.shape
    xp = _pad(x, k, s)
    ho = (xp.shape[1] - k) // s + 1
    wo = (xp.shape[2] - k) // s + 1
    y = np.zeros((n, ho, wo, w_oihw.shape[0]))
    for dy in range(k):
        for dx in range(k):
            patch = xp[:, dy:dy + (ho - 1) * s + 1:s, dx:dx + (wo - 1) * s + 1:s, :]
            y += patch.reshape(-1, c).dot(w_oihw[:, :, dy, dx].T).reshape(y.shape)
    return y


def maxpool(x, k, s):
    """net/layers.py:70-81: stride > 1 pads zeros behind (they take part in the max), stride 1 clips the window at the edge"""
    n, h, w, c = x.shape
    fill = 0.0 if s > 1 else -np.inf
    xp = np.pad(x, ((0, 0), (0, k - 1), (0, k - 1), (0, 0)), constant_values=fill)
    ho = (xp.shape[1] - k) // s + 1
    wo = (xp.shape[2] - k) // s + 1
    y = None
    for dy in range(k):
        for dx in range(k):
            v = xp[:, dy:dy + (ho - 1) * s + 1:s, dx:dx + (wo - 1) * s + 1:s, :]
            y = v if y is None else np.maximum(y, v)
    return np.ascontiguousarray(y)


def reorg(x, s):
    """net/layers.py:90-97, block-major space-to-depth: out[n, i, j, (di*s+dj)*C + c] = in[n, s*i+di, s*j+dj, c]"""
    n, h, w, c = x.shape
    return x.reshape(n, h // s, s, w // s, s, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, h // s, w // s, s * s * c)


def upsample(x, s):
    return x.repeat(s, axis=1).repeat(s, axis=2)


def round_f16(v):
    """float32 -> fp16 (round to nearest even) -> float32"""
    return v.astype(np.float16).astype(np.float32)


def trunc_f16(v):
    """MUTATION: float32 -> fp16 by dropping the low mantissa bits (round toward zero; normal range only)"""
    bits = np.ascontiguousarray(v, np.float32).view(np.uint32) & np.uint32(0xFFFFE000)
    return bits.view(np.float32).astype(np.float16).astype(np.float32)


def folded(wd):
    """float64 fold of weights.cpp pack_weights / forward_ref._conv_folded_fp16 -> (kernel float64 [o][i][kh][kw], bias float32)"""
    w = wd["kernel_oihw"].astype(np.float64)
    if "gamma" in wd:
        scale = wd["gamma"].astype(np.float64) / np.sqrt(wd["var"].astype(np.float64) + 1e-5)
        bias = wd["beta"].astype(np.float64) - wd["mean"].astype(np.float64) * scale
        w = w * scale[:, None, None, None]
    else:
        bias = wd["bias"].astype(np.float64)
    return w, bias.astype(np.float32)


# ---- the reference ------------------------------------------------------------------------------------------------------------
def forward_exact(L, case, dtype, keep=None, stats=None, mutate=None, audit=None, last_shortcut_f32=False):
    """Final output (float32 NHWC) of the layer list on the integer case; with keep (a set of layer indices) also a dict of those.

    dtype "fp16" / "mxfp8": graph input, folded kernels and every stored tensor but the head are fp16 (storage_rules); "fp32": nothing
    is rounded.  stats (dict, filled per conv / shortcut): fp16 ties (odd integers in (2048, 4096) in front of a rounding) and values
    on leaky's negative branch.  mutate: ("drop", layer, (n, y, x, co), (dy, dx, ci)) | ("shift", layer, (n, y), (dy, dx)) |
    ("trunc", layer) -- the deliberate errors of test_exact_cpu.py.  audit (dict): what check_preconditions needs.
    last_shortcut_f32: a shortcut that is the LAST layer is not rounded (what the library does: the fused add goes to the caller's float32
    tensor; forward_ref.forward(storage="fp16") rounds it -- DESIGN.md section 4).
    """
    q16 = dtype in ("fp16", "mxfp8")
    fused, head = storage_rules(L) if q16 else (set(), set())
    outs = [None] * len(L)
    mut = mutate or (None, None)

    def store(i, v):
        """the one rounding of a store"""
        if stats is not None:
            a = np.abs(v)
            st = stats.setdefault(i, {"ties": 0, "neg": 0})
            st["ties"] += int(np.count_nonzero((a > 2048) & (a < 4096) & (np.mod(a, 2) == 1))) if q16 else 0
        if not q16:
            return v
        if audit is not None:
            audit.setdefault("stored_max", {})[i] = float(np.max(np.abs(v)))
        return trunc_f16(v) if mut[0] == "trunc" and mut[1] == i else round_f16(v)

    for i, op in enumerate(L):
        k = op[0]
        if k == "input":
            y = np.asarray(case["x"], np.float32)
            if q16:
                y = round_f16(y)
        elif k == "conv":
            _, src, f, ks, s, bn, act = op
            x = outs[src].astype(np.float64)
            w, bias = folded(case["weights"][i])
            w = w.astype(np.float32)
            if q16:
                w = round_f16(w)
            w = w.astype(np.float64)
            acc = conv_int(x, w, ks, s)
            if mut[0] == "drop" and mut[1] == i:
                (n_, y_, x_, co), (dy, dx, ci) = mut[2], mut[3]
                acc[n_, y_, x_, co] -= _pad(x, ks, s)[n_, y_ * s + dy, x_ * s + dx, ci] * w[co, ci, dy, dx]
            if mut[0] == "shift" and mut[1] == i:       # one tap of one output row reads its neighbour one column to the right
                (n_, y_), (dy, dx) = mut[2], mut[3]
                xp = np.pad(_pad(x, ks, s), ((0, 0), (0, 0), (0, 1), (0, 0)))
                wo = acc.shape[2]
                good = xp[n_, y_ * s + dy, dx:dx + (wo - 1) * s + 1:s, :]
                bad = xp[n_, y_ * s + dy, dx + 1:dx + 1 + (wo - 1) * s + 1:s, :]
                acc[n_, y_] += (bad - good).dot(w[:, :, dy, dx].T)
            if audit is not None:
                bound = conv_int(np.abs(x), np.abs(w), ks, s) + np.abs(bias.astype(np.float64))
                audit.setdefault("bound", {})[i] = float(bound.max())
                audit.setdefault("conv_in", {})[i] = (src, float(np.max(np.abs(x))), bool(np.all(x == np.rint(x))))
                audit.setdefault("w_int", {})[i] = bool(np.all(w == np.rint(w))) and bool(np.all(bias == np.rint(bias)))
                audit.setdefault("w_max", {})[i] = float(np.max(np.abs(w)))
            acc = acc + bias.astype(np.float64)
            if audit is not None:
                audit.setdefault("preact_min", {})[i] = float(acc.min())
            y = acc.astype(np.float32)              # exact: |acc| < 2^24 (check_preconditions)
            if act == "leaky":
                if stats is not None:
                    stats.setdefault(i, {"ties": 0, "neg": 0})["neg"] += int(np.count_nonzero(y < 0))
                y = np.maximum(LEAKY * y, y)        # float32 x float32, one rounding
            if i not in fused and i not in head:
                y = store(i, y)
        elif k == "maxpool":
            y = maxpool(outs[op[1]], op[2], op[3])
        elif k == "route":
            y = outs[op[1][0]] if len(op[1]) == 1 else np.concatenate([outs[j] for j in op[1]], axis=3)
        elif k == "reorg":
            y = reorg(outs[op[1]], op[2])
        elif k == "upsample":
            y = upsample(outs[op[1]], op[2])
        elif k == "shortcut":
            y = outs[op[1]] + outs[op[2]]               # float32 add, then the one rounding
            if not (last_shortcut_f32 and i == len(L) - 1):
                y = store(i, y)
        else:
            raise ValueError("exact_ref does not model %r" % (k,))
        outs[i] = np.ascontiguousarray(y, np.float32)
    res = outs[-1]
    if keep is not None:
        return res, {i: outs[i] for i in keep}
    return res


# ---- data ---------------------------------------------------------------------------------------------------------------------
def make_case(L, batch, seed=0, xmax=8, wmax=8, bmax=3000, hidden_x=3, x_signed=None, growth=3):
    """Seeded integer data for the layer list L at a batch size.

    A conv whose values reach a later conv is HIDDEN: non-negative kernels and biases on a non-negative input, so leaky's negative
    branch (non-integers) never enters a chain; its kernel is as dense as keeps every output <= min(2048, growth x the ACTUAL input maximum)
    (ones, or ones and twos where K is short).  Every other conv is LAST: signed kernels in [-w, w] and signed biases in [-bmax, bmax],
    w <= wmax shrunk (then thinned) until the expected output spread is ~3000, so that fp16 ties in (2048, 4096) and the negative
    branch are hit.  The graph input is signed in [-xmax, xmax] when only LAST convs read it, else in [0, hidden_x].
    BN layers: gamma 1, mean 0, beta = the integer bias, var = float32(1 - 1e-5).
    The density / magnitude rules are heuristics; check_preconditions is what guards a case, so they cannot make a test pass wrongly.
    What they cost: HIDDEN layers see only weights in {0, 1, 2} on small non-negative inputs, so a dropped product there shows only where
    the mask is set.  Signed single-layer probes make up for it for first.hip and the pooled tiles; stem.hip's first two convs are
    exercised with hidden-layer data only.
    Returns {"x", "weights": {layer: parse_darknet_weights-style dict}, "stream": flat float32 in synth.darknet_stream's order}.
    """
    rng = np.random.RandomState(seed)
    S = topology.shapes(L)
    hidden = feeds_conv(L)
    cons = consumers(L)
    if x_signed is None:
        x_signed = not any(op[0] == "conv" and i in hidden for i, op in enumerate(L))
    h, w, c = S[0]
    x = rng.randint(-xmax, xmax + 1, (batch, h, w, c)) if x_signed else rng.randint(0, hidden_x + 1, (batch, h, w, c))
    case = {"x": x.astype(np.float32), "weights": {}}
    outs = [None] * len(L)          # values on the paths into later convs: integers, so no rounding is involved
    parts = []
    for i, op in enumerate(L):
        kind = op[0]
        if kind != "conv" and kind != "input" and i not in hidden:
            continue                    # nothing a conv reads
        if kind == "input":
            outs[i] = case["x"].astype(np.float64)
        elif kind == "maxpool":
            outs[i] = maxpool(outs[op[1]], op[2], op[3])
        elif kind == "route":
            outs[i] = np.concatenate([outs[j] for j in op[1]], axis=3)
        elif kind == "reorg":
            outs[i] = reorg(outs[op[1]], op[2])
        elif kind == "upsample":
            outs[i] = upsample(outs[op[1]], op[2])
        elif kind == "shortcut":
            outs[i] = outs[op[1]] + outs[op[2]]
        elif kind != "conv":
            raise ValueError("exact_ref does not model %r" % (kind,))
        if kind != "conv":
            continue
        _, src, f, ks, s, bn, act = op
        xin = outs[src]
        cin = S[src][2]
        K = ks * ks * cin
        amax = max(1.0, float(np.max(np.abs(xin))))
        if i in hidden:
            b_hi = 4
            # outputs grow by at most `growth` per hidden conv, and a residual sum this conv takes part in stays <= 2048 as well
            cap = CHAIN_MAX
            for j in cons.get(i, []):
                if L[j][0] == "shortcut":
                    other = L[j][2] if L[j][1] == i else L[j][1]
                    cap = min(cap, CHAIN_MAX - int(np.max(outs[other])) if outs[other] is not None else CHAIN_MAX // 4)
            cap = min(cap, max(24, int(growth * amax)))
            room = int((cap - b_hi) // amax)
            assert room >= 1, "layer %d: input maximum %g leaves no room below %d" % (i, amax, cap)
            two = room >= 2 * K
            nnz = min(K, room // 2 if two else room)
            wk = np.zeros((f, K), np.float32)
            for o in range(f):
                wk[o, rng.choice(K, nnz, replace=False)] = 1
            if two:
                wk *= rng.randint(1, 3, wk.shape)
            bias = rng.randint(0, b_hi + 1, f).astype(np.float32)
        else:
            arms = max(1e-3, float(np.sqrt(np.mean(np.square(xin)))))
            wm, dens = wmax, 1.0
            while wm > 1 and arms * wm * 0.61 * np.sqrt(K) > 3000:      # rms of uniform integers in [-w, w] ~ 0.61 w
                wm -= 1
            while arms * wm * 0.61 * np.sqrt(K * dens) > 3000 and dens * K > 4:
                dens *= 0.5
            wk = rng.randint(-wm, wm + 1, (f, K)).astype(np.float32)
            if dens < 1.0:
                wk *= rng.random_sample(wk.shape) < dens
            bias = rng.randint(-bmax, bmax + 1, f).astype(np.float32)
        kern = np.ascontiguousarray(wk.reshape(f, ks, ks, cin).transpose(0, 3, 1, 2))      # [o][i][kh][kw]
        if bn:
            d = {"beta": bias, "gamma": np.ones(f, np.float32), "mean": np.zeros(f, np.float32), "var": np.full(f, BN_VAR, np.float32)}
            parts += [d["beta"], d["gamma"], d["mean"], d["var"]]
        else:
            d = {"bias": bias}
            parts.append(bias)
        d["kernel_oihw"] = kern
        parts.append(kern.reshape(-1))
        case["weights"][i] = d
        if i in hidden:
            y = conv_int(xin, kern.astype(np.float64), ks, s) + bias.astype(np.float64)
            outs[i] = y                 # (non-negative: leaky is the identity)
    case["stream"] = np.concatenate(parts).astype(np.float32)
    return case


# ---- preconditions ------------------------------------------------------------------------------------------------------------
def check_preconditions(L, case, dtype, want_ties=False, want_neg=False, keep=None, **fw):
    """Asserts, from the reference and the data alone, what makes bit equality a theorem for this case; returns
    {"ties", "neg", "bound"}: fp16 ties in front of a rounding, values on leaky's negative branch, largest conv(|x|, |w|) + |b|
    (and, with keep, "out" / "kept": the reference's output of the same pass)."""
    audit, stats = {}, {}
    res = forward_exact(L, case, dtype, stats=stats, audit=audit, keep=keep, **fw)
    q16 = dtype in ("fp16", "mxfp8")
    hidden = feeds_conv(L)
    x = np.asarray(case["x"])
    assert x.dtype == np.float32 and np.all(x == np.rint(x)) and np.max(np.abs(x)) <= CHAIN_MAX, "graph input: integers up to 2048"
    for i, op in enumerate(L):
        if op[0] != "conv":
            continue
        wd = case["weights"][i]
        kern = wd["kernel_oihw"]
        assert np.all(kern == np.rint(kern)) and np.max(np.abs(kern)) <= CHAIN_MAX, "layer %d: integer kernels" % i
        if "gamma" in wd:
            assert np.all(wd["gamma"] == 1) and np.all(wd["mean"] == 0) and np.all(wd["var"] == BN_VAR) and np.all(wd["beta"] == np.rint(wd["beta"]))
        assert audit["w_int"][i], "layer %d: the folded kernel / bias is not integer valued" % i
        w64, _ = folded(wd)
        assert np.array_equal(w64.astype(np.float32), kern) and np.array_equal(w64.astype(np.float32).astype(np.float16).astype(np.float32), kern), \
            "layer %d: the float64 fold does not return the integers" % i
        assert audit["bound"][i] < F24, "layer %d: conv(|x|, |w|) + |b| = %g >= 2^24: a partial sum could round" % (i, audit["bound"][i])
        src, in_max, in_int = audit["conv_in"][i]
        assert in_int, "layer %d reads non-integers (leaky's negative branch upstream?)" % i
        if src != 0:
            assert in_max <= CHAIN_MAX, "layer %d reads |v| = %g > 2048: not exact in fp16" % (i, in_max)
        if i in hidden and op[6] == "leaky":
            assert audit["preact_min"][i] >= 0, "hidden layer %d reaches leaky's negative branch" % i
        if dtype == "mxfp8" and i in mx_candidates(L):
            assert in_max <= MX_MAX and audit["w_max"][i] <= MX_MAX, "layer %d: MX operands above %d" % (i, MX_MAX)
            _check_mx_identity(np.transpose(kern, (0, 2, 3, 1)))
            _check_mx_identity(forward_exact(L[:src + 1], case, dtype) if src else x)
    if q16:
        for i, m in audit.get("stored_max", {}).items():
            assert m < F16_MAX, "layer %d stores %g: beyond fp16" % (i, m)
    ties = sum(s["ties"] for s in stats.values())
    neg = sum(s["neg"] for s in stats.values())
    if want_ties:
        assert ties > 0, "no fp16 tie (odd integer in (2048, 4096)) in front of a rounding"
    if want_neg:
        assert neg > 0, "no value on leaky's negative branch"
    rep = {"ties": ties, "neg": neg, "bound": max(audit["bound"].values())}
    if keep is not None:
        rep["out"], rep["kept"] = res
    return rep


def _check_mx_identity(v):
    """the torch restatement's quantize + dequantize, and the library's own host quantizer + dequantize, return v (last dim % 32 == 0)"""
    import torch
    import mx_ref
    from tensorflow_yolo_amd import _hip
    v = np.ascontiguousarray(v, np.float32)
    rows = v.reshape(-1, v.shape[-1])
    if rows.shape[0] > 4096:                                   # a seeded sample of rows keeps big activations cheap
        rows = rows[np.random.RandomState(0).choice(rows.shape[0], 4096, replace=False)]
    rows = np.ascontiguousarray(rows)
    t = torch.from_numpy(rows)
    assert torch.equal(mx_ref.mx_round(t), t), "mx_round is not the identity"
    q = np.zeros(rows.shape, np.uint8)
    s = np.zeros((rows.shape[0], rows.shape[1] // 32), np.uint8)
    _hip.check(_hip.lib().yolo_mx_quantize_host(rows.ctypes.data, rows.shape[0], rows.shape[1], q.ctypes.data, s.ctypes.data), "yolo_mx_quantize_host")
    assert torch.equal(mx_ref.dequantize(torch.from_numpy(q), torch.from_numpy(s)), t), "yolo_mx_quantize_host + dequantize is not the identity"
