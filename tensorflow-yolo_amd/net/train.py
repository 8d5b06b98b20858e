"""`--mode train` for the detection layer: the reference's loop (net/yolo.py:98-195) around yolo_net_train_head_step.

Runs only when [TRAIN] has `train_layers = head` (a v2 network), `train_layers = tail` (a v2 network: the last 3 x 3 block -- its kernel
and beta; gamma and the moving statistics stay frozen -- and the detection layer, through yolo_net_train_tail_step; checkpoints replace the
block's kernel and beta and the head at their stream positions) or `train_layers = heads` (a v3 network: the convs in front of its
[yolo] layers, trained with the YOLOv3 loss through yolo_net_train_head_step_v3; `ignore_thresh`, default 0.7, is its ignore threshold and
`pretrained_classes = N` lets a file trained for N classes start a fine-tune for another number) or `train_layers = head_blocks` (a v3
network: those convs and the 3 x 3 block behind each -- its kernel and beta --, through yolo_net_train_blocks_step_v3; the other keys as
with `heads`; checkpoints replace every block's kernel and beta and every detection conv at their stream positions).  Two deliberate differences from the reference (include/yolo_hip.h):
only the last conv's kernel and bias receive updates, and the backbone's batch norms run on their stored statistics -- a fine-tune of the
detection layer on a frozen, pretrained backbone.  Batching is the reference's (net/v2.py:209-219: the last batch is padded with the
first annotations, the list is shuffled per epoch), the console lines are its strings, the validation loss is its number (the
yolo_loss_reduce path of Yolo.evaluate).  Checkpoints are Darknet .weights files, `<checkpoint_dir>/<prefix>-<step>.weights`: the
pretrained stream with the head's floats replaced by the master values.  No TensorBoard, no TensorFlow checkpoints.

Augmentation (the reference's imgaug pipeline, net/base.py:15-23, :100-112, :134-135) runs on the device when [TRAIN] has
`augment = device`: then `0 < augment_probability <= 1` is accepted, every training batch is augmented from the resized uint8 batch into a
second buffer (HipNetwork.augment_u8) and its truths are transformed on the host (net/augment.py), with parameters drawn from a generator
of their own seeded by `seed`.  Validation batches are never augmented (the reference's augment_prob = 0).  Without the key a non-zero
probability is refused as before.
"""
import os
import random
import re

import numpy as np

from .. import _hip
from . import base, engine, v3

NOT_SUPPORTED = "train mode is not supported by the HIP inference backend"


def train_layers(params):
    """The [TRAIN] key `train_layers`: absent -> None, `head` (the detection layer of a v2 network), `tail` (its last 3 x 3 block and the
    detection layer), `heads` (the detection convs of a v3 network) or `head_blocks` (those and the 3 x 3 block behind each) -> that word,
    anything else raises ValueError."""
    raw = params.get("train_layers")
    if raw is None:
        return None
    word = str(raw).strip().lower()
    if word not in ("head", "heads", "tail", "head_blocks"):
        raise ValueError("train_layers must be head (the detection layer on a frozen backbone), tail (the last 3 x 3 block and the detection "
                         "layer of a v2 network) or, for a v3 network, heads (its detection convs) or head_blocks (those and the 3 x 3 block "
                         "behind each), got %r" % (raw,))
    return word


def train_option(params):
    """The [TRAIN] key `train_layers`: absent -> False (train keeps raising), `head` or `heads` -> True, anything else raises ValueError."""
    return train_layers(params) is not None


def wgrad_option(params):
    """The [TRAIN] key `wgrad`: absent or `fp32` -> False (yolo_conv3x3_wgrad, today's steps), `fp16` -> True (yolo_conv3x3_wgrad_f16 in the
    tail and blocks steps), anything else raises ValueError."""
    raw = params.get("wgrad")
    if raw is None:
        return False
    word = str(raw).strip().lower()
    if word not in ("fp32", "fp16"):
        raise ValueError("wgrad must be fp32 (the float32 3 x 3 weight gradient) or fp16 (its fp16-operand form), got %r" % (raw,))
    return word == "fp16"


def augment_option(params):
    """The [TRAIN] key `augment`: absent -> False, `device` -> True (augmentation on the device), anything else raises ValueError."""
    raw = params.get("augment")
    if raw is None:
        return False
    if str(raw).strip().lower() != "device":
        raise ValueError("augment must be device (the augmentation kernel), got %r" % (raw,))
    return True


def check_params(params, version):
    """What the head training refuses, before a network is built: a v3 network (the reference binds no loss to YoloV3,
    net/yolo.py:208-211), any augmentation without `augment = device`, and with it a probability outside [0, 1].
    `train_layers = heads` is the other way round: a v3 network only, a v2 network is a ValueError.
    -> the augmentation probability that will run (0.0: none)"""
    if train_layers(params) in ("heads", "head_blocks"):
        if not str(version).startswith("v3"):
            if train_layers(params) == "head_blocks":
                raise ValueError("train_layers = head_blocks trains the detection convs of a v3 network and the 3 x 3 blocks behind them; a %s "
                                 "network takes train_layers = tail" % version)
            raise ValueError("train_layers = heads trains the detection convs of a v3 network; a %s network takes train_layers = head" % version)
        ignore = float(params.get("ignore_thresh", 0.7))
        if not 0 < ignore <= 1:
            raise ValueError("ignore_thresh must be in (0, 1] (got %s)" % params.get("ignore_thresh"))
    elif train_layers(params) == "tail" and not str(version).startswith("v2"):
        raise ValueError("train_layers = tail trains the last 3 x 3 block and the detection layer of a v2 network; a %s network takes "
                         "train_layers = heads" % version)
    elif not str(version).startswith("v2"):
        raise NotImplementedError(NOT_SUPPORTED + " for %s networks: the reference has a loss for YOLOv2 only"
                                  " (train_layers = heads trains the detection convs of a v3 network)" % version)
    if wgrad_option(params):
        if train_layers(params) not in ("tail", "head_blocks"):
            raise ValueError("wgrad = fp16 is the weight gradient of the trained 3 x 3 blocks: it goes with train_layers = tail or head_blocks, "
                             "not with train_layers = %s (no 3 x 3 block is trained)" % train_layers(params))
        if str(params.get("dtype", "fp32")).strip().lower() == "fp32":
            raise ValueError("wgrad = fp16 reads the block's input as the plan stores it, in fp16: it needs dtype = fp16 (a float32 plan stores "
                             "float32 activations)")
    prob = float(params.get("augment_probability", 0))
    if not augment_option(params):
        if prob != 0:
            raise ValueError("augment_probability must be 0: augmentation is not built (got %s)" % params.get("augment_probability"))
        return 0.0
    if not 0 <= prob <= 1:
        raise ValueError("augment_probability must be in [0, 1] with augment = device (got %s)" % params.get("augment_probability"))
    return prob


def make_batches(annotations, batch_size, rng):
    """net/v2.py:209-219: the batch shrinks to a smaller set, the list is padded IN PLACE with its first annotations up to a whole number
    of batches, then shuffled in place with `rng` (a random.Random; the reference uses the module's generator).  -> list of batches"""
    if len(annotations) == 0:
        return []
    if len(annotations) < batch_size:
        batch_size = len(annotations)
    total_batches = int(np.ceil(len(annotations) / batch_size))
    if len(annotations) % batch_size > 0:
        annotations.extend(annotations[0:batch_size - len(annotations) % batch_size])
    rng.shuffle(annotations)
    return [annotations[b * batch_size:(b + 1) * batch_size] for b in range(total_batches)]


def head_counts(net):
    """(cout, cin, floats of the head in the Darknet stream, floats of the whole stream) of a v2 layer list"""
    from .layers import conv2d_bn_act
    convs = [l for l in net if isinstance(l, conv2d_bn_act)]
    need = sum(l.weight_count() for l in convs)
    n_head = convs[-1].weight_count()
    cout = int(net[-1].out.hwc[2])
    cin = (n_head - cout) // cout
    if cout * (cin + 1) != n_head:
        raise ValueError("the last conv is not a 1 x 1 conv with bias")
    return cout, cin, n_head, need


def split_head(body, cout, cin):
    """the head's (kernel [cout, cin], bias [cout]) at the end of a Darknet stream: bias first, then kernel[out][in] (net/layers.py:53-63)"""
    n_head = cout * (cin + 1)
    tail = np.asarray(body[len(body) - n_head:], dtype=np.float32)
    return tail[cout:].reshape(cout, cin).copy(), tail[:cout].copy()


def replace_head(body, w, b):
    """a copy of the stream with the head's floats replaced"""
    out = np.array(body, dtype=np.float32, copy=True)
    cout, cin = w.shape
    n_head = cout * (cin + 1)
    out[len(out) - n_head:len(out) - n_head + cout] = np.asarray(b, dtype=np.float32)
    out[len(out) - cout * cin:] = np.asarray(w, dtype=np.float32).reshape(-1)
    return out


def tail_counts(net):
    """(cout3, cin3, position of the block's first float in the Darknet stream, floats of the block) of a v2 layer list: the block is the
    conv in front of the detection layer, 3 x 3 with batch norm -- beta, gamma, moving mean, moving variance [cout3 each], then the kernel
    [out][in][kh][kw] (net/layers.py:53-63)"""
    from .layers import conv2d_bn_act
    convs = [l for l in net if isinstance(l, conv2d_bn_act)]
    if len(convs) < 2:
        raise ValueError("the network has no conv in front of the detection layer")
    _, _, n_head, need = head_counts(net)
    blk = convs[-2]
    cout3, cin3 = int(blk.filters), int(blk.in_channels)
    if not blk.batch_norm or blk.ksize != 3 or blk.weight_count() != cout3 * (4 + 9 * cin3):
        raise ValueError("the conv in front of the detection layer is not a 3 x 3 conv with batch norm")
    return cout3, cin3, need - n_head - blk.weight_count(), blk.weight_count()


def split_tail(body, net):
    """(the block's piece of the stream, head kernel [cout, cin], head bias [cout]) of a v2 Darknet stream"""
    cout, cin, _, _ = head_counts(net)
    _, _, pos, n_block = tail_counts(net)
    w, b = split_head(body, cout, cin)
    return np.asarray(body[pos:pos + n_block], dtype=np.float32).copy(), w, b


def replace_tail(body, net, kernel3, beta, w, b):
    """a copy of the stream with the block's kernel ([cout3, cin3, 3, 3], the stream's order) and beta and the head's floats replaced at
    their positions; gamma and the moving statistics stay as they are"""
    cout3, cin3, pos, _ = tail_counts(net)
    out = replace_head(body, w, b)
    out[pos:pos + cout3] = np.asarray(beta, dtype=np.float32).reshape(cout3)
    out[pos + 4 * cout3:pos + 4 * cout3 + cout3 * cin3 * 9] = np.asarray(kernel3, dtype=np.float32).reshape(cout3 * cin3 * 9)
    return out


def initial_stream(body, net, seed):
    """The stream training starts from: a full file as it is; a backbone-only file (it ends exactly where the head conv begins, such as
    darknet19_448.conv.23) gets a seeded N(0, 0.02) head kernel and a zero bias.  Anything else raises."""
    cout, cin, n_head, need = head_counts(net)
    body = np.asarray(body, dtype=np.float32)
    if len(body) == need:
        return body, False
    if len(body) == need - n_head:
        w = np.random.RandomState(seed).normal(0.0, 0.02, size=(cout, cin)).astype(np.float32)
        return replace_head(np.concatenate([body, np.zeros(n_head, dtype=np.float32)]), w, np.zeros(cout, dtype=np.float32)), True
    raise ValueError("weight file holds {} values, the network needs {} ({} without the detection layer)".format(len(body), need, need - n_head))


def head_convs_v3(net):
    """The detection convs of a v3 layer list, in head order: [(position of the conv's bias in the Darknet stream, cout, cin)].  A
    detection conv is the conv in front of a yolo layer: its cout biases stand at the position, its kernel [cout][cin] behind them."""
    from .layers import conv2d_bn_act, yolo_layer
    out, pos = [], 0
    for i, l in enumerate(net):
        if not isinstance(l, conv2d_bn_act):
            continue
        if i + 1 < len(net) and isinstance(net[i + 1], yolo_layer):
            if l.batch_norm or l.ksize != 1 or l.weight_count() != l.filters * (l.in_channels + 1):
                raise ValueError("the conv in front of a yolo layer is not a 1 x 1 conv with bias")
            out.append((pos, l.filters, l.in_channels))
        pos += l.weight_count()
    if not out:
        raise ValueError("the network has no yolo layers")
    return out


def split_heads(body, heads):
    """([kernel [cout, cin]], [bias [cout]]) of the detection convs `heads` (head_convs_v3) in a Darknet stream"""
    body = np.asarray(body, dtype=np.float32)
    return ([body[pos + cout:pos + cout * (cin + 1)].reshape(cout, cin).copy() for pos, cout, cin in heads],
            [body[pos:pos + cout].copy() for pos, cout, cin in heads])


def replace_heads(body, heads, ws, bs):
    """a copy of the stream with the floats of the detection convs replaced at their positions"""
    out = np.array(body, dtype=np.float32, copy=True)
    for (pos, cout, cin), w, b in zip(heads, ws, bs):
        out[pos:pos + cout] = np.asarray(b, dtype=np.float32).reshape(cout)
        out[pos + cout:pos + cout * (cin + 1)] = np.asarray(w, dtype=np.float32).reshape(cout * cin)
    return out


def block_convs_v3(net):
    """The 3 x 3 blocks behind the detection convs of a v3 layer list, in head order: [(position of the block's first float -- its beta --
    in the Darknet stream, cout3, cin3)].  The block is the conv in front of a detection conv: 3 x 3 with batch norm -- beta, gamma, moving
    mean, moving variance [cout3 each], then the kernel [out][in][kh][kw] (net/layers.py:53-63)."""
    from .layers import conv2d_bn_act, yolo_layer
    out, pos, prev = [], 0, None
    for i, l in enumerate(net):
        if not isinstance(l, conv2d_bn_act):
            continue
        if i + 1 < len(net) and isinstance(net[i + 1], yolo_layer):
            if prev is None or net[i - 1] is not prev[1]:
                raise ValueError("the layer in front of a detection conv is not a conv")
            blk = prev[1]
            cout3, cin3 = int(blk.filters), int(blk.in_channels)
            if not blk.batch_norm or blk.ksize != 3 or blk.weight_count() != cout3 * (4 + 9 * cin3):
                raise ValueError("the conv in front of a detection conv is not a 3 x 3 conv with batch norm")
            out.append((prev[0], cout3, cin3))
        prev = (pos, l)
        pos += l.weight_count()
    if not out:
        raise ValueError("the network has no yolo layers")
    return out


def split_blocks(body, blocks):
    """[each block's piece of the stream] of the blocks `blocks` (block_convs_v3) in a Darknet stream"""
    body = np.asarray(body, dtype=np.float32)
    return [body[pos:pos + cout3 * (4 + 9 * cin3)].copy() for pos, cout3, cin3 in blocks]


def replace_blocks(body, blocks, kernels, betas):
    """a copy of the stream with every block's kernel ([cout3, cin3, 3, 3], the stream's order) and beta replaced at their positions; gamma
    and the moving statistics stay as they are"""
    out = np.array(body, dtype=np.float32, copy=True)
    for (pos, cout3, cin3), k3, beta in zip(blocks, kernels, betas):
        out[pos:pos + cout3] = np.asarray(beta, dtype=np.float32).reshape(cout3)
        out[pos + 4 * cout3:pos + 4 * cout3 + cout3 * cin3 * 9] = np.asarray(k3, dtype=np.float32).reshape(cout3 * cin3 * 9)
    return out


def replace_head_blocks(body, blocks, heads, kernels, betas, ws, bs):
    """replace_blocks and replace_heads in one: what HipNetwork.blocks_train_read_v3 returns, back into the stream"""
    return replace_heads(replace_blocks(body, blocks, kernels, betas), heads, ws, bs)


def initial_stream_v3(body, net, pretrained_net, seed):
    """The stream a `heads` training starts from.  A stream of exactly the net's length is used as it is.  With pretrained_net -- the same
    network built for the [TRAIN] key `pretrained_classes` = N classes -- a stream of THAT network's length keeps every float outside
    the detection convs, and the detection convs get seeded N(0, 0.02) kernels and zero biases: how an 80-class file starts a 3-class
    fine-tune.  Any other length raises with the lengths in the message.  -> (stream, whether the heads were drawn)"""
    heads = head_convs_v3(net)
    need = sum(l.weight_count() for l in net if hasattr(l, "weight_count"))
    body = np.asarray(body, dtype=np.float32)
    if len(body) == need:
        return body, False
    other = None
    if pretrained_net is not None:
        old = head_convs_v3(pretrained_net)
        other = sum(l.weight_count() for l in pretrained_net if hasattr(l, "weight_count"))
        if len(body) == other:
            out = np.zeros(need, dtype=np.float32)
            src = dst = 0
            for (p_old, co_old, ci_old), (p_new, co_new, ci_new) in zip(old, heads):        # the floats between the detection convs
                out[dst:dst + (p_old - src)] = body[src:p_old]
                assert dst + (p_old - src) == p_new and ci_old == ci_new
                src, dst = p_old + co_old * (ci_old + 1), p_new + co_new * (ci_new + 1)
            out[dst:] = body[src:]
            rng = np.random.RandomState(seed)
            ws = [rng.normal(0.0, 0.02, size=(cout, cin)).astype(np.float32) for _, cout, cin in heads]
            return replace_heads(out, heads, ws, [np.zeros(cout, dtype=np.float32) for _, cout, _ in heads]), True
    raise ValueError("weight file holds {} values, the network needs {}{}".format(
        len(body), need, " ({} with pretrained_classes = the file's class count)".format(other) if other is not None
        else " (no pretrained_classes key: a file trained for another number of classes needs it)"))


def checkpoint_path(checkpoint_dir, prefix, step):
    return os.path.join(checkpoint_dir, "{}-{}.weights".format(prefix, step))


def write_checkpoint(path, header, body):
    """a Darknet v2 .weights file: the pretrained file's four header words, then the stream"""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        np.asarray(header, dtype=np.int32).tofile(f)
        np.ascontiguousarray(body, dtype=np.float32).tofile(f)


def latest_checkpoint(checkpoint_dir, prefix):
    """(step, path) of the `<prefix>-<step>.weights` file with the largest step, or (-1, None) (net/base.py:49-61 load_checkpoint)"""
    best = (-1, None)
    if os.path.isdir(checkpoint_dir):
        for name in os.listdir(checkpoint_dir):
            m = re.match(re.escape(prefix) + r"-(\d+)\.weights$", name)
            if m and int(m.group(1)) > best[0]:
                best = (int(m.group(1)), os.path.join(checkpoint_dir, name))
    return best


def batch_to_device(eng, batch, augment=None):
    """a batch of (image_path, truths) -> (uint8 device tensor [B, H, W, 3] stretched to the network input, truths per image).
    augment = (random.Random, probability): one record per image in batch order (net/augment.py: draw), the resized batch augmented into
    a second buffer, the truths transformed with the same records (stretch: frame-normalised truths are input-normalised too)."""
    descs, keep = eng.frame_descs(base.decode_frames([p for p, _ in batch]))
    x = eng.preprocess_frames(descs, len(batch), _hip.RESIZE_STRETCH, u8=True)
    eng._frames_keep = keep
    truths = [t for _, t in batch]
    if augment is not None and augment[1] > 0:
        from . import augment as yaug
        h, w, _ = eng.input_hwc
        records = [yaug.draw(augment[0], augment[1], h, w) for _ in batch]
        x = eng.augment_u8(x, records)
        truths = [yaug.truths(p, t, h, w) for p, t in zip(records, truths)]
    return x, truths


def validation_loss(eng, annotations, batch_size):
    """net/yolo.py:177-193 on the device: per-image partials of every image (HipNetwork.loss_u8), added once (yolo_loss_reduce) with the
    padding of make_batch counted twice, divided by the number of batches.  One read."""
    from . import evaluate as yeval
    torch = eng.torch
    n = len(annotations)
    bs, nb, pad = yeval.loss_batches(n, batch_size)
    images = torch.empty((n, yeval.LOSS_IMAGE_DTYPE.itemsize), dtype=torch.uint8, device=eng.device)
    for start in range(0, n, bs):
        x, truths = batch_to_device(eng, annotations[start:start + bs])
        eng.loss_u8(x, truths, images=images[start:start + len(truths)])
    total = torch.empty(yeval.LOSS_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=eng.device)
    with torch.cuda.device(eng.device):
        _hip.check(eng.lib.yolo_loss_reduce(images.data_ptr(), n, pad, bs, total.data_ptr(), eng._stream()), "yolo_loss_reduce")
    rec = total.cpu().numpy().view(yeval.LOSS_RESULT_DTYPE)[0]
    return float(rec["loss"]) / nb


def validation_loss_v3(eng, annotations, batch_size, ignore_thresh):
    """validation_loss for a v3 network: the per-image partials of HipNetwork.loss_v3_u8, added and weighted the same way"""
    from . import evaluate as yeval
    torch = eng.torch
    n = len(annotations)
    bs, nb, pad = yeval.loss_batches(n, batch_size)
    images = torch.empty((n, yeval.LOSS_IMAGE_DTYPE.itemsize), dtype=torch.uint8, device=eng.device)
    for start in range(0, n, bs):
        x, truths = batch_to_device(eng, annotations[start:start + bs])
        eng.loss_v3_u8(x, truths, ignore_thresh, images=images[start:start + len(truths)])
    total = torch.empty(yeval.LOSS_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=eng.device)
    with torch.cuda.device(eng.device):
        _hip.check(eng.lib.yolo_loss_reduce(images.data_ptr(), n, pad, bs, total.data_ptr(), eng._stream()), "yolo_loss_reduce")
    rec = total.cpu().numpy().view(yeval.LOSS_RESULT_DTYPE)[0]
    return float(rec["loss"]) / nb


def train_head(model, params):
    """Yolo.train with `train_layers = head` or `tail` (a v2 network) or `heads` or `head_blocks` (a v3 network): one loop, the entries of
    the version"""
    from . import evaluate as yeval
    augment_prob = check_params(params, model.version)
    v3_heads = train_layers(params) in ("heads", "head_blocks")
    v3_blocks = train_layers(params) == "head_blocks"
    tail = train_layers(params) == "tail"
    ignore_thresh = float(params.get("ignore_thresh", 0.7))
    batch_size = int(params["batch_size"])
    learning_rate = float(params["learning_rate"])
    checkpoint_prefix, checkpoint_dir = params["checkpoint_prefix"], params["checkpoint_dir"]
    checkpoint_step = int(params["checkpoint_step"])
    anchors = np.reshape(params["anchors"], [-1, 2])
    class_names = params["class_names"]
    input_shape = (int(params["input_h"]), int(params["input_w"]), int(params["input_c"]))
    epochs, max_step = int(params["epochs"]), int(params["max_step"])
    seed = int(params.get("seed", 0))
    if params.get("tensorboard_log_dir"):
        print("tensorboard_log_dir is ignored: this backend writes no TensorBoard summaries")
    if str(params.get("cpu_only", "false")).lower() == "true":
        print("cpu_only = True is ignored: this backend runs on the MI355X only")

    train_annotations, _ = yeval.parse_voc_annotations(params["annotation_dir"], params["image_dir"], class_names)
    assert len(train_annotations) > 0
    val_annotations, _ = yeval.parse_voc_annotations(params["val_annotation_dir"], params["val_image_dir"], class_names)

    model.build(anchors, class_names, input_shape, dtype=params.get("dtype", "fp32"), max_batch=batch_size, streams=1)
    net, eng = model.net, model.net.engine
    file_version = "v3" if v3_heads else "v2"
    if v3_heads:
        heads = head_convs_v3(net)
    else:
        cout, cin, _, _ = head_counts(net)
    header, pretrained = base.read_darknet_weights(params["pretrained_weights_path"], file_version)
    step, path = latest_checkpoint(checkpoint_dir, checkpoint_prefix)
    if step < 0:
        if v3_heads:
            old = None
            if params.get("pretrained_classes") is not None:
                names = ["c%d" % i for i in range(int(params["pretrained_classes"]))]
                old = type(model).create_network(anchors, names, False, input_shape=tuple(input_shape))
            body, drawn = initial_stream_v3(pretrained, net, old, seed)
        else:
            body, drawn = initial_stream(pretrained, net, seed)
        v3.attach_weights(net, body)
        print("Pre-trained weights loaded." + (" Detection layer drawn from N(0, 0.02), seed {}.".format(seed) if drawn else ""))
        step = 0
        write_checkpoint(checkpoint_path(checkpoint_dir, checkpoint_prefix, step), header, body)
    else:
        header, body = base.read_darknet_weights(path, file_version)
        v3.attach_weights(net, body)
        print("Checkpoint restored. step:{}".format(step))
    # (the moments are not part of a .weights file: they start at zero)
    if v3_blocks:
        blocks = block_convs_v3(net)
        eng.blocks_train_init_v3(split_blocks(body, blocks), *split_heads(body, heads))
        read_stream = lambda: replace_head_blocks(body, blocks, heads, *eng.blocks_train_read_v3())
        step_u8 = lambda x, truths, lr_t, result: eng.train_blocks_step_v3_u8(x, truths, lr_t, ignore_thresh, result=result)
        val_loss = lambda: validation_loss_v3(eng, val_annotations, batch_size, ignore_thresh)
    elif v3_heads:
        eng.head_train_init_v3(*split_heads(body, heads))
        read_stream = lambda: replace_heads(body, heads, *eng.head_train_read_v3())
        step_u8 = lambda x, truths, lr_t, result: eng.train_head_step_v3_u8(x, truths, lr_t, ignore_thresh, result=result)
        val_loss = lambda: validation_loss_v3(eng, val_annotations, batch_size, ignore_thresh)
    elif tail:
        eng.tail_train_init(*split_tail(body, net))
        read_stream = lambda: replace_tail(body, net, *eng.tail_train_read())
        step_u8 = lambda x, truths, lr_t, result: eng.train_tail_step_u8(x, truths, lr_t, result=result)
        val_loss = lambda: validation_loss(eng, val_annotations, batch_size)
    else:
        eng.head_train_init(*split_head(body, cout, cin))
        read_stream = lambda: replace_head(body, *eng.head_train_read())
        step_u8 = lambda x, truths, lr_t, result: eng.train_head_step_u8(x, truths, lr_t, result=result)
        val_loss = lambda: validation_loss(eng, val_annotations, batch_size)

    rng = random.Random(seed)
    augment = None
    if augment_prob > 0:
        from . import augment as yaug
        augment = (yaug.stream(seed), augment_prob)
        print("Augmentation on the device with probability {}.".format(augment_prob))
    if wgrad_option(params):
        eng.set_wgrad_f16(True)
        print("3 x 3 weight gradients on the fp16 matrix cores.")
    result = eng.torch.empty(yeval.LOSS_RESULT_DTYPE.itemsize, dtype=eng.torch.uint8, device=eng.device)
    train_loss_mva, updates = None, 0
    for epoch in range(1, epochs + 1):
        if 0 <= max_step < step:
            break
        for batch in make_batches(train_annotations, batch_size, rng):
            step += 1
            if 0 <= max_step < step:
                break
            updates += 1
            x, truths = batch_to_device(eng, batch, augment)
            step_u8(x, truths, engine.adam_lr_t(learning_rate, updates), result)
            train_loss = np.float32(result.cpu().numpy().view(yeval.LOSS_RESULT_DTYPE)[0]["loss"])
            train_loss_mva = train_loss_mva * 0.9 + train_loss * 0.1 if train_loss_mva is not None else train_loss
            print("step {} ({}/{}): {} (moving average: {})".format(step, epoch, epochs, train_loss, train_loss_mva))
            if step > 0 and step % checkpoint_step == 0:
                write_checkpoint(checkpoint_path(checkpoint_dir, checkpoint_prefix, step), header, read_stream())
                if val_annotations:
                    print("validation loss: {}".format(val_loss()))
                else:
                    print("no validation annotations: validation skipped")
        print("Epoch ({}/{}) completed.".format(epoch, epochs))
    if v3_blocks:
        model.trained_blocks = eng.blocks_train_read_v3()
        model.trained_head = model.trained_blocks[2:]
    elif tail:
        model.trained_tail = eng.tail_train_read()
        model.trained_head = model.trained_tail[2:]
    else:
        model.trained_head = eng.head_train_read_v3() if v3_heads else eng.head_train_read()
    print("Done")
