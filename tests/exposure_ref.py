"""float64 numpy restatement of the exposure correction (ibgs_amd/exposure.py; the reference's compute_exposure_affine_matrix,
color_aggregation_network.py:136-153, 182-185) -- the ARBITER of tests/test_gpu_exposure.py -- and the float32 YARDSTICK: the reference's own formulation
(boolean gather, cat, torch.linalg.lstsq, einsum) in float32 torch, whose distance from the arbiter is the measure of what float32 can be asked for."""
import numpy as np
import torch


def first_slot(warped_image):
    """(3 S, H, W) or (S, 3, H, W) -> the 3 planes of slot 0."""
    w = np.asarray(warped_image)
    return w[:3] if w.ndim == 3 else w[0]


def design(render, mask):
    """-> the N x 4 design matrix [r0 r1 r2 1] of the pixels whose mask word is 1 (float64), and the boolean (H, W) selection."""
    sel = np.asarray(mask).reshape(np.asarray(render).shape[1:]) == 1
    r = np.asarray(render, np.float64)[:, sel]
    return np.concatenate([r, np.ones((1, r.shape[1]))], 0).T, sel


def determined(render, mask, rcond=1e-9):
    """The rule of include/ibgs_exposure.h, stated independently: at least 4 pixels, and a design matrix of full column rank after its columns are scaled
    to unit length (singular values of the scaled matrix; the device tests pivots of its Gram matrix, the squares).  The cases the tests use are far from
    the threshold on either side."""
    x, _ = design(render, mask)
    if x.shape[0] < 4:
        return False
    norm = np.linalg.norm(x, axis=0)
    if not np.all(norm > 0):
        return False
    s = np.linalg.svd(x / norm, compute_uv=False)
    return bool(s[-1] > rcond * s[0])


def fit_ref(render, warped_image, mask):
    """-> (affine (3, 4) float64, fit_ok).  numpy.linalg.lstsq on the masked pixels; [I | 0] and False where the fit is undetermined."""
    x, sel = design(render, mask)
    if not determined(render, mask):
        return np.concatenate([np.eye(3), np.zeros((3, 1))], 1), False
    y = np.asarray(first_slot(warped_image), np.float64)[:, sel].T
    return np.linalg.lstsq(x, y, rcond=None)[0].T, True


def apply_ref(affine, image):
    """corrected[i] = A[i,0] r0 + A[i,1] r1 + A[i,2] r2 + A[i,3], float64."""
    a, r = np.asarray(affine, np.float64), np.asarray(image, np.float64)
    return np.einsum("ij,jhw->ihw", a[:, :3], r) + a[:, 3, None, None]


def apply_backward_ref(affine, grad):
    """d render[j] = sum_i A[i,j] g[i], float64 (the affine map is a constant)."""
    return np.einsum("ij,ihw->jhw", np.asarray(affine, np.float64)[:, :3], np.asarray(grad, np.float64))


def correct_ref(render, warped_image, mask):
    """-> (corrected (3, H, W) float64, affine, fit_ok); an undetermined fit returns render itself."""
    a, ok = fit_ref(render, warped_image, mask)
    return (apply_ref(a, render) if ok else np.asarray(render, np.float64)), a, ok


def cond(render, mask):
    """The condition number of the design matrix."""
    return float(np.linalg.cond(design(render, mask)[0]))


def torch_composition(render, warped_image, mask, dtype=torch.float32):
    """The reference's lines in torch at `dtype`, on the tensors' device: first_warped * mask, the boolean gather, cat, lstsq under no_grad, einsum.
    -> (corrected (3, H, W), affine (3, 4)); differentiable in render through the einsum alone, as there."""
    h, w = render.shape[-2:]
    i_r = render.to(dtype)
    valid = mask.reshape(1, h, w)
    i_s = warped_image.reshape(-1, 3, h, w)[0].to(dtype) * valid
    with torch.no_grad():
        sel = (valid == 1)[0]
        r_valid, s_valid = i_r[:, sel], i_s[:, sel]
        x = torch.cat([r_valid, torch.ones((1, r_valid.shape[1]), device=i_r.device, dtype=dtype)], 0).T
        # driver "gels" is what the reference runs (the only one torch has on the device); the CPU's default, gelsy, truncates the rank at eps * max(N, 4)
        # and would drop the near-grey directions of a large frame
        affine = torch.linalg.lstsq(x, s_valid.T, driver="gels").solution.T
    aug = torch.cat([i_r, torch.ones((1, h, w), device=i_r.device, dtype=dtype)], 0)
    return torch.einsum("ij,jhw->ihw", affine, aug), affine


def yardstick(render, warped_image, mask, upstream=None):
    """The float32 yardstick on the CPU from numpy inputs: -> (corrected, affine[, d render for `upstream`]) as float32 numpy arrays."""
    r = torch.tensor(np.asarray(render, np.float32), requires_grad=upstream is not None)
    out, a = torch_composition(r, torch.tensor(np.asarray(warped_image, np.float32)), torch.tensor(np.asarray(mask, np.int32)))
    if upstream is None:
        return out.detach().numpy(), a.numpy()
    g, = torch.autograd.grad((out * torch.tensor(np.asarray(upstream, np.float32))).sum(), r)
    return out.detach().numpy(), a.numpy(), g.numpy()


def case(h, w, density, grey=False, seed=0, s=2):
    """Seeded inputs: render in [0, 1] (near-grey: the channels differ by about 1e-3), warped slot 0 an affine image of render plus noise, the other slots
    random, a mask with words 0, 1 and 2 of which `density` are 1 (density 1: all).  -> render (3, H, W), warped (S, 3, H, W), mask (1, H, W) int32."""
    rng = np.random.default_rng(1000 * seed + 31 * h + w + (7 if grey else 0) + int(100 * density))
    if grey:
        render = rng.uniform(0.05, 0.95, (1, h, w)) + 1e-3 * rng.standard_normal((3, h, w))
    else:
        render = rng.uniform(0, 1, (3, h, w))
    true = np.array([[0.9, 0.06, -0.03, 0.02], [0.04, 1.1, 0.05, -0.03], [-0.02, 0.03, 0.8, 0.05]])
    warped = rng.uniform(0, 1, (s, 3, h, w))
    warped[0] = apply_ref(true, render) + 0.02 * rng.standard_normal((3, h, w))
    u = rng.uniform(0, 1, (1, h, w))
    mask = np.where(u < density, 1, np.where(u < density + (1 - density) / 2, 0, 2)).astype(np.int32)
    return render.astype(np.float32), warped.astype(np.float32), mask
