"""What the geometry units (knn, tsdf, mesh, mesh_eval, registration, dtu) share on the Python side: how the library is called on a tensor's device and
stream, how CPU tensors are refused, how state words and scratch are allocated, and the argument checks for clouds and positive numbers.  The modules of
the training step (rasterizer, renderer, optim, ...) do not come through here: their host path is timed."""
import math

import numpy as np
import torch

from . import _lib

MAX_POINTS = (1 << 31) - 1


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def call(dev, name, *args):
    """lib.<name>(torch's current stream on dev, *args) with dev current; a negative return raises with the library's message."""
    with torch.cuda.device(dev):
        rc = getattr(_lib.load(), name)(stream(dev), *args)
    if rc < 0:
        raise RuntimeError("%s failed (%d): %s" % (name, rc, _lib.last_error()))


def refuse_cpu(module, name, t):
    if not t.is_cuda:
        raise RuntimeError("ibgs_amd.%s runs on the MI355X only (%s is a CPU tensor; there is no CPU path)" % (module, name))


def check_cuda(module, *named):
    """After every shape and value check: (name, tensor) pairs must be device tensors on one device.  -> the tensors, contiguous."""
    for name, t in named:
        refuse_cpu(module, name, t)
    for name, t in named[1:]:
        if t.device != named[0][1].device:
            raise ValueError("%s is on %s, %s on %s" % (named[0][0], named[0][1].device, name, t.device))
    return [t.contiguous() for _, t in named]


def zeros_state(dev, words):
    """A unit's state words (int32), zeroed."""
    return torch.zeros(words, dtype=torch.int32, device=dev)


def scratch(dev, nbytes):
    """A caller-owned arena: torch's allocations are 128-byte aligned, which is what the library asks for."""
    with torch.cuda.device(dev):
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)


def check_points(name, p):
    if not torch.is_tensor(p):
        raise TypeError("%s must be a tensor, got %s" % (name, type(p).__name__))
    if p.dtype != torch.float32 or p.dim() != 2 or p.shape[1] != 3:
        raise ValueError("%s must be (N, 3) float32, got %s %s" % (name, tuple(p.shape), p.dtype))
    if p.shape[0] > MAX_POINTS:
        raise ValueError("%s holds %d points (limit: N < 2^31)" % (name, p.shape[0]))
    return p


def check_positive(name, x, allow_zero=False):
    try:
        x = float(x)
    except (TypeError, ValueError):
        raise TypeError("%s must be a number, got %s" % (name, type(x).__name__)) from None
    if not math.isfinite(x) or x < 0 or (x == 0 and not allow_zero) or float(np.float32(x)) > 1e18:
        raise ValueError("%s must be a finite %s number, got %r" % (name, "non-negative" if allow_zero else "positive", x))
    return x
