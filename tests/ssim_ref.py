"""Restatement of the reference's SSIM map (utils/loss_utils.py:24-32, 44-59, 66-91) that autograd can differentiate, on any device and in any float
type, in the three forms the fused kernel (ibgs_amd/csrc/ssim.hip) is judged by:

  "shift2d"    the reference's float32 2-D window -- the outer product of its float32 1-D weights, rounded to float32, then cast to `dtype` -- applied by
               121 shifted adds over the zero-padded planes.  At float64 this is the ARBITER: nothing in it depends on a convolution backend.
  "conv2d"     the same window through F.conv2d(groups=C): the reference's own call.  On the GPU it runs under `torch_own_conv()`, forward and backward: torch's own
               kernels (depthwise; im2col + GEMM for a single channel), not MIOpen's solvers.  MIOpen picks a solver per shape (direct, Winograd, composable-kernel or its naive fallback), and on the
               small odd planes of the parity cases (one pixel wide, smaller than the window) a backward through them ended the test process with an abort on one
               box while passing on others; the formulation under test -- 121 float32 products of the rounded 2-D window summed per pixel -- is the same.
  "separable"  the float32 1-D weights cast to `dtype`, 11 shifted adds along the rows, then 11 down the columns.  A separable kernel applies g_i g_j
               unrounded where the reference rounds each product to float32: a property of the formulation, not of a kernel.

The yardstick of a quantity is the larger of the distances of "conv2d" and "separable" at float32 from the arbiter; the kernel may be F64_K = 2 times as far
(tests/test_gpu_ssim.py).  Pinned on the CPU against tests/metrics.ssim and the reference's own numbers by tests/test_ssim_host.py."""
import contextlib
from math import exp

import torch
import torch.nn.functional as F

WINDOW, SIGMA, HALF = 11, 1.5, 5
C1, C2 = 0.01 ** 2, 0.03 ** 2
F64_K = 2.0          # the project's factor on a float32 yardstick (tests/test_gpu_anisotropic.py:23)
FORMS = ("shift2d", "conv2d", "separable")


@contextlib.contextmanager
def torch_own_conv():
    """F.conv2d and its backward inside this block do not go through MIOpen (see "conv2d" above).  The backward picks its implementation when it RUNS:
    torch.autograd.grad / backward() of a "conv2d" map belong inside the block too."""
    old = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    try:
        yield
    finally:
        torch.backends.cudnn.enabled = old


def gaussian():
    """loss_utils.py:24-26: exp in double, stored as float32, divided by their float32 sum."""
    g = torch.Tensor([exp(-(x - WINDOW // 2) ** 2 / float(2 * SIGMA ** 2)) for x in range(WINDOW)])
    return g / g.sum()


def window_2d():
    """loss_utils.py:29-30, float32."""
    w = gaussian().unsqueeze(1)
    return w.mm(w.t()).float()


def blur(x, form):
    """x: (N, C, H, W) -> w * x with zero padding of 5, in x's dtype."""
    n, c, h, w = x.shape
    if form == "conv2d":
        k = window_2d().to(device=x.device, dtype=x.dtype).expand(c, 1, WINDOW, WINDOW).contiguous()
        if x.is_cuda:
            backend = torch._C._select_conv_backend(x, k, None, (1, 1), (HALF, HALF), (1, 1), False, (0, 0), c).name
            if "Miopen" in backend or "Cudnn" in backend:          # (expected: CudaDepthwise2d, and Slow2d for a single channel)
                raise RuntimeError("ssim_ref: the conv2d form on the GPU runs inside torch_own_conv() (torch would use %s here)" % backend)
        return F.conv2d(x, k, padding=HALF, groups=c)
    p = F.pad(x, (HALF, HALF, HALF, HALF))
    if form == "shift2d":
        k = window_2d().to(torch.float64).tolist()          # (a Python float holds a float32 exactly; the product below is formed in x's dtype)
        out = None
        for i in range(WINDOW):
            for j in range(WINDOW):
                t = k[i][j] * p[:, :, i:i + h, j:j + w]
                out = t if out is None else out + t
        return out
    if form == "separable":
        g = gaussian().to(torch.float64).tolist()
        row = None
        for j in range(WINDOW):
            t = g[j] * p[:, :, :, j:j + w]
            row = t if row is None else row + t
        out = None
        for i in range(WINDOW):
            t = g[i] * row[:, :, i:i + h, :]
            out = t if out is None else out + t
        return out
    raise ValueError(form)


def ssim_map_ref(a, b, dtype=torch.float64, form="shift2d"):
    """The SSIM map of a, b ((C, H, W) or (N, C, H, W)) in `dtype`, in the input's shape; differentiable in both."""
    shape = a.shape
    x = a.to(dtype).reshape((-1,) + tuple(shape[-3:]))
    y = b.to(dtype).reshape((-1,) + tuple(shape[-3:]))
    mu1, mu2 = blur(x, form), blur(y, form)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = blur(x * x, form) - mu1_sq
    s2 = blur(y * y, form) - mu2_sq
    s12 = blur(x * y, form) - mu1_mu2
    m = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return m.reshape(shape)


def run(a, b, dtype, form, loss_of_map, wrt=(0,)):
    """-> (map, loss, [gradients with respect to the images named in wrt]) of `form` at `dtype`, all as float64.  loss_of_map(m) -> a scalar in m's dtype."""
    ins = [t.detach().to(dtype).requires_grad_(k in wrt) for k, t in enumerate((a, b))]
    with torch_own_conv():
        m = ssim_map_ref(ins[0], ins[1], dtype, form)
        loss = loss_of_map(m)
        grads = torch.autograd.grad(loss, [ins[k] for k in wrt]) if wrt else []
    return m.detach().double(), loss.detach().double(), [g.double() for g in grads]


def arbiter_and_yardstick(a, b, loss_of_map, wrt=(0,)):
    """-> (map64, loss64, grads64, d_map, [d_grad]): the arbiter's results and, per quantity, the larger max-abs distance of the two float32 forms from them."""
    m64, l64, g64 = run(a, b, torch.float64, "shift2d", loss_of_map, wrt)
    d_map, d_grad = 0.0, [0.0] * len(wrt)
    for form in ("conv2d", "separable"):
        m, _, g = run(a, b, torch.float32, form, loss_of_map, wrt)
        d_map = max(d_map, float((m - m64).abs().max()))
        d_grad = [max(d, float((gi - gj).abs().max())) for d, gi, gj in zip(d_grad, g, g64)]
    return m64, l64, g64, d_map, d_grad
