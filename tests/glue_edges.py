"""Helpers for the edge tests of the fused glue kernels (ibgs_amd/csrc/depth_normal.hip, loss.hip, activate.hip).

Depth -> normal: the cases (image sizes around the backward's 64 x 8 LDS tile, zero-depth holes), the reference (`renderer.normal_from_depth_image` plus
render()'s normalisation, float64 on the CPU), the pixel classes a halo / seam / partial-tile / clamp-branch error would land in, and the per-class bar

    rel L2 (candidate vs float64) <= max(K * rel L2 (torch fp32 vs float64), 1e-6)         over the pixels of ONE class,

so that an error confined to one row or column per tile is not diluted by the rest of the image.  The floor is always torch's own fp32 evaluation of the
formulation, never the candidate's.  tests/test_glue_edges_host.py runs all of it on the CPU with a second fp32 evaluation standing in for the kernel.

Buffers: `Guarded` places an array inside a larger allocation whose padding holds a recognisable NaN, for the C ABI calls of tests/test_gpu_glue_bounds.py."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from ibgs_amd import renderer
from tests.metrics import rel_l2

TILE_W, TILE_H = 64, 8          # DN_TW, DN_TH of depth_normal_bwd_kernel
HUGE = 1e10                     # |dL/ddepth| above this only where the clamp of F.normalize decided (a zero cross product on a hole's rim: the reference's 1e-12 * 1e-8 in the denominator)
FLOOR = 1e-6
K_CLASS = 2.0                   # the project's whole-image factor (tests/test_gpu_depth_normal.py), applied per class

# (r0, r1, c0, c1), inclusive, of the 197 x 29 case: across a column seam (63 | 64) and a row seam (7 | 8); touching the image corner; one pixel; inside the last
# partial tile (u >= 192, v >= 24) up to the right edge
HOLES_197x29 = ((5, 11, 60, 68), (0, 4, 0, 5), (20, 20, 100, 100),(24, 27, 193, 196))

CASES = {
    "197x29 holes": (197, 29, HOLES_197x29),
    "197x29": (197, 29, ()),
    "64x8": (64, 8, ()), "65x9": (65, 9, ()), "128x16": (128, 16, ()), "63x7": (63, 7, ()),
    "3x3": (3, 3, ()), "2x5": (2, 5, ()), "5x2": (5, 2, ()), "2x2": (2, 2, ()),
}


def make_cam(fx, fy, cx, cy):
    c = SimpleNamespace(Fx=fx, Fy=fy, Cx=cx, Cy=cy)
    c.get_calib_matrix_nerf = lambda scale=1.0: (torch.tensor([[fx / scale, 0, cx / scale], [0, fy / scale, cy / scale], [0, 0, 1]]).float(), torch.eye(4))
    return c


def case_cam(W, H):
    """Focal length about the image width (the fp32 cancellation noise of the point differences grows with it), fy != fx, principal point well off the centre."""
    fx = 1.22 * max(W, 8)
    return make_cam(fx, 1.07 * fx, 0.37 * W, 0.61 * H)


def torch_glue(cam, depth):
    """render_normal + the normalisation of render(), in the dtype and on the device of `depth`: the reference formulation."""
    K, _ = cam.get_calib_matrix_nerf()
    n = renderer.normal_from_depth_image(depth, K.to(depth.dtype)).permute(2, 0, 1)
    return n / (torch.norm(n, dim=0, keepdim=True) + 1e-8)


def direct_glue(cam, depth):
    """The same map without the matrix product and its inverse: points as d * (u / fx - cx / fx, v / fy - cy / fy, 1).  Another rounding of the same
    function; the host test uses its fp32 evaluation as a stand-in for the kernel."""
    H, W = depth.shape
    dt, dev = depth.dtype, depth.device
    u = torch.arange(W, dtype=dt, device=dev)[None, :]
    v = torch.arange(H, dtype=dt, device=dev)[:, None]
    p = torch.stack([(u * depth) / cam.Fx - depth * (cam.Cx / cam.Fx), (v * depth) / cam.Fy - depth * (cam.Cy / cam.Fy), depth], dim=-1)
    n = torch.cross(p[1:H - 1, 2:W] - p[1:H - 1, 0:W - 2], p[0:H - 2, 1:W - 1] - p[2:H, 1:W - 1], dim=-1)
    n = torch.nn.functional.normalize(n, p=2, dim=-1)
    n = torch.nn.functional.pad(n.permute(2, 0, 1), (1, 1, 1, 1), mode="constant")
    return n / (torch.norm(n, dim=0, keepdim=True) + 1e-8)


def make_depth(W, H, holes=()):
    """A smooth surface plus noise (as tests/test_gpu_depth_normal.py), 0 inside the holes: what a median-depth map holds where no Gaussian covers the pixel."""
    gen = torch.Generator().manual_seed(1000 * W + H)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    depth = 3.0 + 0.8 * torch.sin(3.0 * xx) * torch.cos(2.0 * yy) + 0.02 * torch.randn(H, W, generator=gen)
    for r0, r1, c0, c1 in holes:
        depth[r0:r1 + 1, c0:c1 + 1] = 0.0
    return depth


def make_cot(W, H, lattice=False):
    cot = torch.randn(3, H, W, generator=torch.Generator().manual_seed(7 + 1000 * W + H))
    if lattice:          # non-zero only where v % 3 == 1 and u % 3 == 1: every pixel is 4-adjacent to at most one of them
        keep = torch.zeros(H, W, dtype=torch.bool)
        keep[1::3, 1::3] = True
        cot = cot * keep
    return cot


def lattice_support(W, H):
    """Pixels 4-adjacent to a lattice pixel: the only ones whose depth enters a normal with a non-zero cotangent."""
    lat = np.zeros((H, W), bool)
    lat[1::3, 1::3] = True
    s = np.zeros((H, W), bool)
    s[1:, :] |= lat[:-1, :]; s[:-1, :] |= lat[1:, :]; s[:, 1:] |= lat[:, :-1]; s[:, :-1] |= lat[:, 1:]
    return s


def _dilate(m, r):
    """Chebyshev dilation by r (pixels outside the image are not set)."""
    H, W = m.shape
    p = np.zeros((H + 2 * r, W + 2 * r), bool)
    p[r:r + H, r:r + W] = m
    out = np.zeros((H, W), bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= p[dy:dy + H, dx:dx + W]
    return out


def pixel_masks(depth):
    """name -> (H, W) bool.  The hole classes partition the neighbourhood of the zero-depth pixels; every other class leaves that neighbourhood out (the
    gradients there reach 1e18 and would own any norm they are part of); the other classes may overlap each other."""
    d = np.asarray(depth)
    H, W = d.shape
    zero = d == 0
    near = _dilate(zero, 2)                      # within Chebyshev distance 2 of a zero-depth pixel
    deep = ~_dilate(~zero, 2)                    # every pixel of the image within distance 2 has depth 0
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    border = (u < 2) | (v < 2) | (u >= W - 2) | (v >= H - 2)
    col = (u % TILE_W == 0) | (u % TILE_W == TILE_W - 1)
    row = (v % TILE_H == 0) | (v % TILE_H == TILE_H - 1)
    part = (u >= TILE_W * (W // TILE_W)) | (v >= TILE_H * (H // TILE_H))
    m = {"hole rim": near & ~deep, "deep hole": deep,
         "column seams": col & ~near, "row seams": row & ~near, "last partial tiles": part & ~near, "border ring": border & ~near,
         "rest": ~(col | row | part | border | near)}
    m["border"] = (u == 0) | (v == 0) | (u == W - 1) | (v == H - 1)          # one pixel wide: the normal is exactly 0 there (not a distance class)
    return m


DISTANCE_CLASSES = ("hole rim", "column seams", "row seams", "last partial tiles", "border ring", "rest")


def gradient_classes(masks, g64):
    """The distance classes for dL/ddepth: the hole rim split by the float64 gradient into the entries the clamp branch made huge and the ordinary ones."""
    out = {}
    for name in DISTANCE_CLASSES:
        if name == "hole rim":
            big = np.abs(g64) > HUGE
            out["hole rim, huge"] = masks[name] & big
            out["hole rim, ordinary"] = masks[name] & ~big
        else:
            out[name] = masks[name]
    return out


def normal_classes(masks):
    return {name: masks[name] for name in DISTANCE_CLASSES}


def evaluate(fn, cam, depth, cot, dtype, device):
    """(normal map, dL/ddepth) of `fn(cam, depth)` under the cotangent `cot`, as float64 numpy arrays."""
    d = depth.detach().to(dtype).to(device).clone().requires_grad_(True)          # (a leaf of its own: `.to` returns its argument when nothing changes)
    out = fn(cam, d)
    (out * cot.to(dtype).to(device)).sum().backward()
    return out.detach().cpu().double().numpy(), d.grad.detach().cpu().double().numpy()


@functools.lru_cache(maxsize=None)
def reference(case, lattice=False):
    """Inputs, masks and the float64 evaluation of one case: computed once, shared by every test that needs it, never written to."""
    W, H, holes = CASES[case]
    cam, depth, cot = case_cam(W, H), make_depth(W, H, holes), make_cot(W, H, lattice)
    n64, g64 = evaluate(torch_glue, cam, depth, cot, torch.float64, "cpu")
    for a in (n64, g64):
        a.setflags(write=False)
    return SimpleNamespace(case=case, W=W, H=H, cam=cam, depth=depth, cot=cot, n64=n64, g64=g64, masks=pixel_masks(depth.numpy()))


def class_distances(tag, cand, floor, ref, classes, K=K_CLASS):
    """Per non-empty class: rel L2 of candidate and of the floor evaluation against the float64 reference.  Prints every row; returns (rows, names of the
    classes over the bar).  Arrays are (H, W) or (3, H, W); the masks are (H, W)."""
    rows, bad = [], []
    for name, m in classes.items():
        if not m.any():
            continue
        e_c, e_f = rel_l2(cand[..., m], ref[..., m]), rel_l2(floor[..., m], ref[..., m])
        bar = max(K * e_f, FLOOR)
        rows.append((name, int(m.sum()), e_c, e_f))
        print("[glue edges] %s | %-20s n=%5d: candidate %.2e, torch fp32 %.2e (ratio %s), bar %.2e%s"
              % (tag, name, int(m.sum()), e_c, e_f, "%.2f" % (e_c / e_f) if e_f > 0 else "-", bar, "" if e_c <= bar else "   <-- OVER"))
        if not e_c <= bar:
            bad.append(name)
    return rows, bad


def structural_zeros(normal, grad, masks):
    """What must hold exactly, for the float64 reference as for the kernel: no normal on the one-pixel border, nothing at all deep inside a hole."""
    problems = []
    if not (np.isfinite(normal).all() and np.isfinite(grad).all()):
        problems.append("non-finite value")
    if (normal[..., masks["border"]] != 0).any():
        problems.append("non-zero normal on the image border")
    if (normal[..., masks["deep hole"]] != 0).any():
        problems.append("non-zero normal deep inside a hole")
    if (grad[masks["deep hole"]] != 0).any():
        problems.append("non-zero dL/ddepth deep inside a hole")
    return problems


# ---- guarded buffers ----------------------------------------------------------------------------------------------------------------------------------

GUARD_WORDS = 16384               # 64 KiB each side
GUARD_BITS = 0x7FC5A5A5           # a quiet NaN no arithmetic produces
FRESH_BITS = 0x7FC3C3C3           # what an output's payload holds before the call: a result still carrying it was never written


class Guarded:
    """`n` fp32 words inside an allocation with GUARD_WORDS of GUARD_BITS before and after.  `data` (a tensor or None) fills the payload of an input;
    an output's payload starts as FRESH_BITS.  `shift` moves the payload by that many words (0: 16-byte aligned, as the allocation is)."""

    def __init__(self, n, data=None, device="cuda", shift=0):
        self.n, self.lo = int(n), GUARD_WORDS + int(shift)
        self.buf = torch.full((self.lo + self.n + GUARD_WORDS,), GUARD_BITS, dtype=torch.int32, device=device)
        self.view = self.buf[self.lo:self.lo + self.n].view(torch.float32)
        if data is None:
            self.buf[self.lo:self.lo + self.n] = FRESH_BITS
        else:
            self.view.copy_(data.reshape(-1).to(torch.float32))
        self.before = self.buf.clone()

    def ptr(self):
        return self.buf.data_ptr() + 4 * self.lo

    def guards_intact(self):
        return bool(torch.equal(self.buf[:self.lo], self.before[:self.lo]) and torch.equal(self.buf[self.lo + self.n:], self.before[self.lo + self.n:]))

    def untouched(self):
        return bool(torch.equal(self.buf, self.before))

    def bits(self):
        return self.buf[self.lo:self.lo + self.n].clone()
