"""YOLOv3 (Darknet-53 + three-scale head), YOLOv3-SPP and YOLOv3-tiny for the HIP backend.

Same three plug points as the reference's net/v3.py -- `create_network` (:9-94), `load_weights`
(:98-106), `find_bounding_boxes` (:140-151) -- with the same signatures; the layer list has the
same 109 entries in the same order, so layer indices (route sources 62 and 37) and the Darknet
weight order carry over.

`create_spp_network` and `create_tiny_network` are NOT in the reference: they are upstream Darknet's yolov3-spp.cfg and yolov3-tiny.cfg
written in the same layer vocabulary (as net/v2.py does for tiny-YOLOv2), with the signature of `create_network`; `load_weights`,
`find_bounding_boxes` and the head decode work on their two or three scales unchanged.
"""
import numpy as np

from .. import _hip
from . import base, engine
from .layers import conv2d_bn_act, detection_layer, input_layer, max_pool2d, route, shortcut, upsample, yolo_layer

# Darknet-53 trunk: (filters of the stride-2 conv, number of residual blocks that follow)
_STAGES = ((64, 1), (128, 2), (256, 8), (512, 8), (1024, 4))
_SKIP_FINE = 36 + 1     # output of the last 256-channel block (+1: the input layer is entry 0)
_SKIP_MID = 61 + 1      # output of the last 512-channel block
_SPP_POOLS = (5, 9, 13)  # stride-1 SAME max-pools of the SPP block (yolov3-spp.cfg)


class Network(list):
    """The layer list plus what the runtime attaches to it."""
    version = "v3"
    engine = None
    darknet_weights = None


def create_network(anchors, class_names, is_training, scope="yolo", input_shape=(416, 416, 3)):
    return _darknet53_network(anchors, class_names, is_training, scope, input_shape, spp=False)


def create_spp_network(anchors, class_names, is_training, scope="yolo", input_shape=(416, 416, 3)):
    """YOLOv3-SPP: `create_network` with a spatial-pyramid-pooling block inside the coarse head -- behind its third conv (1x1, 512
    channels: x) come max-pools 5, 9 and 13 at stride 1 of x, each behind a route back to x, and route [pool13, pool9, pool5, x]
    (2048 channels); then 1x1 512, 3x3 1024, 1x1 512, 3x3 1024 and the head conv.  Darknet weight order = conv order of the list."""
    return _darknet53_network(anchors, class_names, is_training, scope, input_shape, spp=True)


def _darknet53_network(anchors, class_names, is_training, scope, input_shape, spp):
    num_classes = len(class_names)
    per_scale = np.reshape(anchors, [3, -1, 2])[::-1, :, :]     # coarsest head gets the largest anchors
    conv2d_bn_act.reset()
    net = Network()
    kw = dict(is_training=is_training, scope=scope)

    def conv(filters, ksize, stride=1, **extra):
        net.append(conv2d_bn_act(net[-1].out, filters, ksize, stride, **dict(kw, **extra)))

    def residual(filters):
        block_in = net[-1]
        conv(filters // 2, 1)
        conv(filters, 3)
        net.append(shortcut(net[-1].out, block_in.out))

    def head(filters, sub_anchors, spp_block=False):
        if spp_block:
            conv(filters, 1)
            conv(filters * 2, 3)
            conv(filters, 1)
            x = net[-1]
            pools = []
            for k in _SPP_POOLS:
                if pools:
                    net.append(route([x.out]))
                net.append(max_pool2d(net[-1].out, k, stride=1))
                pools.append(net[-1])
            net.append(route([p.out for p in reversed(pools)] + [x.out]))
            conv(filters, 1)
            conv(filters * 2, 3)
            conv(filters, 1)
            conv(filters * 2, 3)
        else:
            for _ in range(3):
                conv(filters, 1)
                conv(filters * 2, 3)
        conv(len(sub_anchors) * (5 + num_classes), 1, 1, use_batch_normalization=False, activation_fn="linear")
        net.append(yolo_layer(net[-1].out, sub_anchors, num_classes, input_shape))
        return net[-1]

    def lateral(filters, skip_index):
        net.append(route([net[-4].out]))            # the 1x1 output two convs before the head conv
        conv(filters, 1)
        net.append(upsample(net[-1].out, 2))
        net.append(route([net[-1].out, net[skip_index].out]))

    net.append(input_layer([None, input_shape[0], input_shape[1], input_shape[2]], "input"))
    conv(32, 3)
    for filters, blocks in _STAGES:
        conv(filters, 3, 2)
        for _ in range(blocks):
            residual(filters)

    yolos = [head(512, per_scale[0], spp_block=spp)]
    lateral(256, _SKIP_MID)
    yolos.append(head(256, per_scale[1]))
    lateral(128, _SKIP_FINE)
    yolos.append(head(128, per_scale[2]))
    net.append(detection_layer(yolos))
    return net


def create_tiny_network(anchors, class_names, is_training, scope="yolo", input_shape=(416, 416, 3)):
    """YOLOv3-tiny (yolov3-tiny.cfg, 13 convs): tiny-YOLOv2's trunk -- 16-32-64-128-256 with 2x2/2 pools, 512 + 2x2/1 pool, 1024 -- and a
    two-scale v3 head: 1x1 256, 3x3 512, head conv at stride 32; route to the 1x1 256, 1x1 128, upsample, route with the 256-channel
    26 x 26 conv, 3x3 256, head conv at stride 16.

    Anchors split as in `create_network` (reshape [2, -1, 2], reversed): the stride-32 head gets anchors 3, 4, 5 of the list, the
    stride-16 head anchors 0, 1, 2.  Some upstream tiny cfgs give mask 1, 2, 3 to the fine head; the anchors are the caller's
    configuration, so such a model lists its six anchors accordingly."""
    num_classes = len(class_names)
    per_scale = np.reshape(anchors, [2, -1, 2])[::-1, :, :]
    conv2d_bn_act.reset()
    net = Network()
    kw = dict(is_training=is_training, scope=scope)

    def conv(filters, ksize, **extra):
        net.append(conv2d_bn_act(net[-1].out, filters, ksize, 1, **dict(kw, **extra)))

    def head(sub_anchors):
        conv(len(sub_anchors) * (5 + num_classes), 1, use_batch_normalization=False, activation_fn="linear")
        net.append(yolo_layer(net[-1].out, sub_anchors, num_classes, input_shape))
        return net[-1]

    net.append(input_layer([None, input_shape[0], input_shape[1], input_shape[2]], "input"))
    for filters in (16, 32, 64, 128, 256):
        conv(filters, 3)
        skip = net[-1]                              # (after the loop: the 256-channel map at stride 16)
        net.append(max_pool2d(net[-1].out, 2, stride=2))
    conv(512, 3)
    net.append(max_pool2d(net[-1].out, 2, stride=1))
    conv(1024, 3)
    conv(256, 1)
    branch = net[-1]
    conv(512, 3)
    yolos = [head(per_scale[0])]
    net.append(route([branch.out]))
    conv(128, 1)
    net.append(upsample(net[-1].out, 2))
    net.append(route([net[-1].out, skip.out]))
    conv(256, 3)
    yolos.append(head(per_scale[1]))
    net.append(detection_layer(yolos))
    return net


def load_weights(layers, weights_path):
    """Reads the Darknet file and hands the float stream to the network's engine (uploaded eagerly;
    nothing is returned to run, unlike the reference's list of tf.assign ops)."""
    print("Reading pre-trained weights from {}".format(weights_path))
    header, weights = base.read_darknet_weights(weights_path, "v3")
    print("{} {} {} {} {}".format(*header))
    print("Found {} weight values.".format(len(weights)))
    return attach_weights(layers, weights)


def attach_weights(layers, weights):
    need = sum(l.weight_count() for l in layers if isinstance(l, conv2d_bn_act))
    if need != len(weights):
        # stricter than the reference, which only prints the two counts (net/base.py:44)
        raise ValueError("weight file holds {} values, the network needs {}".format(len(weights), need))
    layers.darknet_weights = np.ascontiguousarray(weights, dtype=np.float32)
    if layers.engine is not None:
        layers.engine.load_weights(layers.darknet_weights)
    print("Weights ready ({}/{} read)".format(need, len(weights)))
    return []


def find_bounding_boxes(net_out, net, threshold, iou_threshold, anchors, class_names, nms_mode=0):
    """Head decode over the three scales + one NMS per image, on the GPU (libyolo_hip
    yolo_decode_nms).  net_out: [B, rows, 5+C] NumPy array or torch device tensor."""
    head = engine.head_desc_v3(net[-1].yolos)
    eng = getattr(net, "engine", None)
    records, _ = engine.decode_nms(head, net_out, threshold, iou_threshold, nms_mode,
                                   cand_capacity=eng.cand_capacity if eng else 4096,
                                   max_boxes=eng.max_boxes if eng else _hip.DEFAULT_MAX_BOXES)
    return base.boxes_from_records(records)
