"""Command-line entry of the HIP backend.

Keeps the reference launcher's surface (reference launcher.py:15-60): the two flags `--config` and
`--mode` with the same defaults (mode defaults to "anchor", exactly as there), `.ini` sections
COMMON / ANCHOR / TRAIN / TEST merged as {**section, **COMMON}, relative `*_dir` / `*_path` values
resolved against the .ini's directory, `anchors` / `class_names` parsed as Python literals, and the
network picked by COMMON.version.  `test` runs on this backend, and `eval` (not in the reference): VOC-style mAP of the
network on an annotated directory, from an [EVAL] section laid over [TEST] (eval_params); `train` runs when [TRAIN] has
`train_layers = head` (the detection layer on a frozen backbone: net/train.py; `seed` seeds the shuffle and a drawn head; `tail` adds the
last 3 x 3 block of a v2 network, `heads` trains the detection convs of a v3 network, `head_blocks` those and the 3 x 3 block behind
each); `anchor` runs when [ANCHOR] has `kmeans = device` (k-means over the boxes of `annotation_dir` on the device: net/anchors.py; optional
keys `distance` euclidean | iou, `n_init`, `max_iter`, `seed`; prints the reference's four lines, then the run's figures and the anchors as a
list ready for an .ini); otherwise
`train` and `anchor` end with a clear message.  Extra, optional keys: `dtype` (fp32 | fp16 | mxfp8: block-scaled fp8 3x3 convs), `nms_mode` (agnostic | per_class), `max_boxes` / `cand_capacity` (record caps), `autotune` (True: per-layer tile timing at start-up),
`resize` (stretch, the reference's geometry and the default | letterbox, Darknet's: aspect ratio kept, grey canvas, boxes mapped back to the frame),
`loss` ([EVAL] only; true: also report the reference's validation loss, net/yolo.py:177-193 -- YOLOv2, resize = stretch);
version additionally accepts `v2-tiny`, `v3-tiny` and `v3-spp`.  `--section` selects another TEST-like section (the
reference's yolo_2.ini keeps its COCO settings in [TEST_COCO], which no mode reaches there).
"""
import argparse
import ast
import configparser
import os
import sys

_PKG = os.path.dirname(os.path.abspath(__file__))
DEFAULT_CONFIG = os.path.join(_PKG, "config", "yolo_2.ini")
LITERAL_KEYS = ("anchors", "class_names")
PATH_SUFFIXES = ("_dir", "_path")


def resolve_section(values, ini_path):
    """One section's key/value strings -> dict with absolute paths and parsed literals."""
    base = os.path.dirname(os.path.abspath(ini_path))
    out = {}
    for key, value in values.items():
        if key.endswith(PATH_SUFFIXES) and not os.path.isabs(value):
            value = os.path.join(base, value)
        elif key in LITERAL_KEYS:
            value = ast.literal_eval(value)
        out[key] = value
    return out


def read_config(ini_path):
    parser = configparser.ConfigParser()
    if not parser.read(ini_path):
        raise IOError("cannot read config file {}".format(ini_path))
    return {name: resolve_section(dict(parser.items(name)), ini_path) for name in parser.sections()}


def pick_model(version):
    from .net.yolo import YoloV2, YoloV2Tiny, YoloV3, YoloV3SPP, YoloV3Tiny
    table = {"v2": YoloV2, "v3": YoloV3, "v2-tiny": YoloV2Tiny, "v3-tiny": YoloV3Tiny, "v3-spp": YoloV3SPP}
    if version not in table:
        raise ValueError("Unsupported version: {}".format(version))
    return table[version]()


def test_options(params):
    """The optional TEST keys with a closed set of values, checked before a network is built: `resize` (stretch | letterbox).
    Returns them parsed; anything else raises ValueError."""
    from . import _hip
    return {"resize": _hip.resize_mode(params.get("resize", "stretch"))}


def eval_options(params):
    """test_options plus the optional [EVAL] key `loss` (true | false: also report the reference's validation loss; YOLOv2 and
    resize = stretch only), checked before a network is built.  Returns them parsed; anything else raises ValueError."""
    from .net import evaluate
    out = test_options(params)
    out["loss"] = evaluate.loss_option(params, params.get("version", ""))
    return out


EVAL_DEFAULTS = {"threshold": "0.005", "max_boxes": "1024", "match_iou": "0.5"}


def eval_params(cfg, section=None):
    """`--mode eval`: the [TEST] keys (or those of --section), overridden by [EVAL] -- `annotation_dir`, `image_dir`, `match_iou` and
    whatever else it sets -- then [COMMON].  threshold and max_boxes default to a mAP run's 0.005 and 1024 unless [EVAL] sets them
    (the [TEST] values are a demo's).  Raises ValueError without an [EVAL] section or its two directories."""
    if "EVAL" not in cfg:
        raise ValueError("mode 'eval' needs an [EVAL] section with annotation_dir and image_dir")
    params = dict(cfg.get(section or "TEST", {}))
    params.update(EVAL_DEFAULTS)
    params.update(cfg["EVAL"])
    params.update(cfg["COMMON"])
    for key in ("annotation_dir", "image_dir"):
        if key not in cfg["EVAL"]:
            raise ValueError("[EVAL] needs {}".format(key))
    m = float(params["match_iou"])
    if not 0. <= m <= 1.:
        raise ValueError("match_iou must be in [0, 1], got {}".format(params["match_iou"]))
    return params


def run(cfg, mode, section=None):
    yolo = pick_model(cfg["COMMON"]["version"])
    if mode == "test":
        params = dict(cfg[section or "TEST"])
        params.update(cfg["COMMON"])
        test_options(params)
        yolo.test(params)
    elif mode == "eval":
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:      # (Yolo.evaluate itself is not sharded: every caller scores the whole set)
            raise SystemExit("mode 'eval' runs in one process: sharded evaluation needs a merge of the records, which is not built")
        params = eval_params(cfg, section)
        eval_options(params)
        yolo.evaluate(params)
    elif mode == "train" and "train_layers" in cfg.get("TRAIN", {}):      # the detection layer on a frozen backbone (net/train.py)
        from .net import train as ytrain
        params = dict(cfg["TRAIN"])
        params.update(cfg["COMMON"])
        ytrain.train_option(params)
        ytrain.check_params(params, cfg["COMMON"]["version"])
        yolo.train(params)
    elif mode == "anchor" and "kmeans" in cfg.get("ANCHOR", {}):          # k-means on the device (net/anchors.py)
        from .net import anchors as yanchors
        params = dict(cfg["ANCHOR"])
        params.update(cfg["COMMON"])
        yanchors.anchor_option(params)
        yanchors.check_params(params, cfg["COMMON"]["version"])
        anchors, class_names = yolo.generate_anchors(params)
        print("Anchors: ")
        print("\t{}".format(anchors))
        print("Class names: ")
        print("\t{}".format(class_names))
        res = yolo.last_anchor_result
        print("distance: {}".format("iou" if res.distance else "euclidean"))
        print("best restart: {} of {}".format(res.best_restart, len(res.restarts)))
        print("iterations: {}".format(res.n_iter))
        print("avg_iou: {:.6f}".format(res.avg_iou))
        print("boxes used: {}, skipped: {}".format(res.n_valid, res.n_bad))
        print("anchors = {}".format([float(v) for v in anchors]))
    elif mode in ("train", "anchor"):
        raise SystemExit("mode '{}' is not supported by the HIP inference backend (TEST mode only)".format(mode))
    else:
        raise ValueError("Unsupported mode: {}".format(mode))


def main(argv=None):
    ap = argparse.ArgumentParser(description="YOLO v2/v3 TEST-mode inference on MI355X")
    ap.add_argument("--config", dest="config", help="Path to configuration file", default=DEFAULT_CONFIG)
    ap.add_argument("--mode", dest="mode", help="Mode: (train|test|anchor|eval)", default="anchor")
    ap.add_argument("--section", dest="section", help="section to use for test mode (default TEST)", default=None)
    args = ap.parse_args(argv)
    group = init_distributed()
    try:
        run(read_config(args.config), args.mode.lower(), args.section)
    finally:
        if group:
            import torch.distributed as dist
            dist.destroy_process_group()


def init_distributed():
    """One process per GPU: under a multi-process launcher (`torchrun launcher.py ...` sets WORLD_SIZE / RANK / LOCAL_RANK /
    MASTER_*) bind this process to its GPU and join the group BEFORE anything touches the device, so that Yolo.test shards
    every batch over the ranks (net/dist.py).  Backend "nccl" (= RCCL) on GPUs, "gloo" where there is none (the CPU tests).
    Returns True when this call created the group."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return False
    import torch
    import torch.distributed as dist
    if dist.is_initialized():
        return False
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    rank, local_rank = int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    if torch.cuda.device_count() > local_rank and torch.cuda.is_available():
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    return True


if __name__ == "__main__":
    if __package__ in (None, ""):       # executed as a script: make the package importable
        sys.path.insert(0, os.path.dirname(_PKG))
        import tensorflow_yolo_amd.launcher as _self
        _self.main()
    else:
        main()
