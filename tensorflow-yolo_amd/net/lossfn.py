"""The reference's YOLOv2 loss as ONE differentiable torch op on the device.

    loss = yolo_v2_loss(logits, truths, anchors, n_classes)
    loss.backward()                 # logits.grad (or whatever produced the logits) receives d loss / d logits

Forward is one call of yolo_v2_loss_grad (include/yolo_hip.h has the definitions): truth assignment (net/v2.py:242-295), every term of
net/v2.py:123-198 and the gradient with respect to the logits -- what tf.gradients hands AdamOptimizer.minimize at net/v2.py:205 -- all
on the device, on the current stream, with no host synchronisation and no dense gt / mask tensors built on the host.  Backward is
`grad_output * G`.  Everything behind the logits (the backward pass of a backbone, the optimizer) is ordinary torch autograd of the
caller's own model; this package has no backward pass through its own networks.
"""
import numpy as np

from . import engine

_FN = None
_FN3 = None


def _function():
    """the torch.autograd.Function, created on first use (importing the package does not import torch)"""
    global _FN
    if _FN is not None:
        return _FN
    import torch
    from torch.autograd.function import once_differentiable

    class YoloV2LossFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, logits, truths, head):
            x = logits.detach().contiguous()
            images, result, assign, grad, keep = engine.v2_loss_grad(head, x, truths)
            ctx.save_for_backward(grad)
            ctx.in_shape = tuple(logits.shape)
            ctx.keep = (x, images, assign) + keep          # (alive until backward: the work is only enqueued)
            loss = result.view(torch.float64)[0].to(torch.float32)     # yolo_loss_result.loss, read on the device
            ctx.mark_non_differentiable(result)
            return loss, result

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_loss, _grad_record):
            grad, = ctx.saved_tensors
            return (grad_loss * grad).reshape(ctx.in_shape), None, None

    _FN = YoloV2LossFn
    return _FN


def yolo_v2_loss(logits, truths, anchors, n_classes, return_record=False):
    """logits: float32 device tensor [B, h, w, A * (5 + C)] or [B, h, w, A, 5 + C] (made contiguous if it is not); truths: a list per
    image of (x, y, w, h, class_idx) normalised to the image, the pair of evaluate.pack_gts, or the device tensors of
    Evaluator.upload_gts; anchors: (w, h) pairs in grid units; n_classes: C.  Returns the loss as a 0-dim float32 device tensor with a
    grad_fn (float32 of the float64 total of yolo_loss_result); with return_record also the 64-byte yolo_loss_result record as a uint8
    device tensor (not differentiable; evaluate.LOSS_RESULT_DTYPE reads it).  ValueError for anything else."""
    import torch
    anchors = np.reshape(np.asarray(anchors, dtype=np.float64), [-1, 2])
    A, width = len(anchors), 5 + int(n_classes)
    if not isinstance(logits, torch.Tensor):
        raise ValueError("logits: expected a float32 device tensor, got %s" % type(logits).__name__)
    shape = tuple(int(v) for v in logits.shape)
    if not ((len(shape) == 4 and shape[3] == A * width) or (len(shape) == 5 and shape[3:] == (A, width))) or shape[0] < 1:
        raise ValueError("logits: expected [B, h, w, %d] or [B, h, w, %d, %d] for %d anchors and %d classes, got %s"
                         % (A * width, A, width, A, int(n_classes), shape))
    if logits.dtype != torch.float32 or logits.device.type != "cuda":
        raise ValueError("logits: expected a float32 device tensor, got %s on %s" % (logits.dtype, logits.device))
    head = engine.head_desc_v2(shape[1], shape[2], anchors, int(n_classes))
    loss, record = _function().apply(logits, truths, head)
    return (loss, record) if return_record else loss


def _function_v3():
    global _FN3
    if _FN3 is not None:
        return _FN3
    import torch
    from torch.autograd.function import once_differentiable

    class YoloV3LossFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, logits, truths, head, ignore_thresh):
            x = logits.detach().contiguous()
            images, result, assign, grad, keep = engine.v3_loss_grad(head, x, truths, ignore_thresh)
            ctx.save_for_backward(grad)
            ctx.in_shape = tuple(logits.shape)
            ctx.keep = (x, images, assign) + keep          # (alive until backward: the work is only enqueued)
            loss = result.view(torch.float64)[0].to(torch.float32)     # yolo_loss_result.loss, read on the device
            ctx.mark_non_differentiable(result)
            return loss, result

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_loss, _grad_record):
            grad, = ctx.saved_tensors
            return (grad_loss * grad).reshape(ctx.in_shape), None, None, None

    _FN3 = YoloV3LossFn
    return _FN3


def yolo_v3_loss(logits, truths, grids, anchors, n_classes, ignore_thresh=0.7, return_record=False):
    """The loss of Darknet's [yolo] layer as ONE differentiable torch op on the device (include/yolo_hip.h has the definition): forward is
    one call of yolo_v3_loss_grad, backward is `grad_output * G`.  logits: float32 device tensor [B, R, 5 + C] in the layout of a version 3
    head's output (made contiguous if it is not), R = sum of h * w * A over the scales; truths as yolo_v2_loss takes them; grids:
    [(h, w), ...] in head order; anchors: per scale a list of (w, h) pairs in the grid units of that scale; n_classes: C; ignore_thresh in
    (0, 1].  Returns the loss as a 0-dim float32 device tensor with a grad_fn; with return_record also the 64-byte yolo_loss_result
    record as a uint8 device tensor (not differentiable).  ValueError for anything else."""
    import torch
    head = engine.head_desc_v3(grids, anchors, n_classes)
    rows, width = sum(head.h[s] * head.w[s] * head.n_anchors[s] for s in range(head.n_scales)), 5 + int(n_classes)
    if not isinstance(logits, torch.Tensor):
        raise ValueError("logits: expected a float32 device tensor, got %s" % type(logits).__name__)
    shape = tuple(int(v) for v in logits.shape)
    if len(shape) != 3 or shape[1:] != (rows, width) or shape[0] < 1:
        raise ValueError("logits: expected [B, %d, %d] for these grids, anchors and %d classes, got %s" % (rows, width, int(n_classes), shape))
    if logits.dtype != torch.float32 or logits.device.type != "cuda":
        raise ValueError("logits: expected a float32 device tensor, got %s on %s" % (logits.dtype, logits.device))
    if not 0. < float(ignore_thresh) <= 1.:
        raise ValueError("ignore_thresh: expected a value in (0, 1], got %r" % (ignore_thresh,))
    loss, record = _function_v3().apply(logits, truths, head, float(ignore_thresh))
    return (loss, record) if return_record else loss
