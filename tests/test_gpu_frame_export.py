"""The frame export (ibgs_amd.frame_export; csrc/export.hip) on the device.

The yardstick is tests/frame_export_ref.py, the numpy restatement that tests/test_frame_export_host.py pins to np.percentile and to the recorded run of the
reference's own colorize.  EVERY comparison here is exact: equal bytes for the images, equal bits for the percentiles.  Nothing has a tolerance."""
import functools
import os

import numpy as np
import pytest
import torch

from ibgs_amd import frame_export as fe
from ibgs_amd import image_eval, losses
from tests import dirty_alloc as da
from tests import frame_export_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_export.npz")
SIZES = [(1, 1), (1, 3), (5, 7), (33, 65)]
CASES = {c[0]: c for c in ref.percentile_cases()}


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = got != want
    assert not bad.any(), "%s: %d of %d elements differ, first at %s: %r against %r" % (what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


def _same_bits(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (what, got, want)


@functools.lru_cache(maxsize=None)
def _lut():
    """The fixture's table on the device; where matplotlib is importable `colormap_lut` builds it instead, and the two are the same table."""
    z = np.load(GOLDEN)
    table = _dev(z["lut"])
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return table
    built = fe.colormap_lut("magma_r", DEV)
    assert built.dtype == torch.uint8 and torch.equal(built, table)
    return built


def _residual(x):
    """a residual from rule inputs: magnitudes up to 3.25 (so that |r| / max |r| spreads over the bytes), the largest, 3.6, in the last element"""
    r = (np.clip(x, -3, 3) - np.float32(0.25)).astype(np.float32)
    r.reshape(-1)[-1] = -3.6
    return r


# ---- rules 1-3 -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SIZES)
def test_to_u8_normal_and_residual_are_the_restatement_byte_for_byte(h, w):
    x = ref.rule_inputs(h, w)
    xd = _dev(x)
    for rule in ("round", "truncate"):
        for order in ("rgb", "bgr"):
            _same(fe.to_u8(xd, rule, order), ref.to_u8(x, rule, order), "to_u8 %s %s" % (rule, order))
        _same(fe.to_u8(xd[1:2], rule), ref.to_u8(x[1:2], rule), "to_u8 %s, one channel" % rule)
    _same(fe.to_u8(xd), ref.to_u8(x), "to_u8 defaults")
    # a view with another stride and another float type: converted, not refused
    _same(fe.to_u8(xd.double().flip(0)), ref.to_u8(x[::-1]), "to_u8 of a flipped float64 view")
    n = (ref.rule_inputs(h, w, seed=1) * np.float32(2) - np.float32(1)).astype(np.float32)
    n.reshape(-1)[:3] = [1.0, -1.0, 1.5][:n.size]          # +-1 and beyond (3 values at least: 3 planes)
    _same(fe.normal_to_u8(_dev(n)), ref.normal_to_u8(n), "normal_to_u8")
    r = _residual(x)
    assert np.abs(r).argmax() == r.size - 1          # the maximum sits in the last element: the scalar tail, or the last lane of the last workgroup
    want, status = ref.residual_vis_u8(r)
    got, st = fe.residual_vis_u8(_dev(r))
    _same(got, want, "residual_vis_u8")
    assert int(st) == status == 0 and st.is_cuda and st.dtype == torch.int32 and want.max() == 255
    _same(fe.residual_vis_u8(_dev(r[:1]))[0], ref.residual_vis_u8(r[:1])[0], "residual_vis_u8, one channel")
    got, st = fe.residual_vis_u8(torch.zeros(3, h, w, device=DEV))
    assert int(st) == ref.ZERO_RESIDUAL and got.dtype == torch.uint8 and tuple(got.shape) == (h, w, 3) and int(got.max()) == 0
    got, st = fe.residual_vis_u8(-torch.zeros(3, h, w, device=DEV))
    assert int(st) == ref.ZERO_RESIDUAL and int(got.max()) == 0
    q = fe.quantize(xd)
    assert q.dtype == torch.float32 and q.shape == xd.shape and np.array_equal(q.cpu().numpy().view(np.uint32), ref.quantize(x).view(np.uint32))


# ---- rule 4 ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_percentile_is_the_restatement_bit_for_bit(name):
    _, v, qs, inv, mask = CASES[name]
    want, status = ref.percentile(v, qs, inv, mask)
    got, st = fe.percentile(_dev(v), qs, inv, None if mask is None else _dev(mask), return_status=True)
    _same_bits(got, want, name)
    assert int(st) == status and st.dtype == torch.int32 and st.is_cuda
    assert (status == ref.NO_VALID) == (name == "all_invalid")
    if v.size % 5 == 0 and v.size > 5:          # the shape does not matter, and the default return is the values alone
        m2 = None if mask is None else _dev(mask).reshape(5, -1)
        _same_bits(fe.percentile(_dev(v).reshape(5, -1), qs, inv, m2), want, name + " as a matrix")


def test_percentile_of_nothing():
    got, st = fe.percentile(torch.zeros(0, device=DEV), (2, 85), return_status=True)
    assert int(st) == ref.NO_VALID and got.cpu().tolist() == [0.0, 0.0]


# ---- rule 5 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_colorize_reproduces_the_reference_run():
    z = np.load(GOLDEN)
    lut = _lut()
    for name in (str(n) for n in z["names"]):
        value = z["in_" + name]
        got, st = fe.colorize(_dev(value), lut, return_status=True)
        _same(got, z["out_" + name], name)
        _same(got, ref.colorize(value, z["lut"])[0], name + " (restatement)")
        assert int(st) == 0
        _same(fe.colorize(_dev(value[0]), lut), z["out_" + name], name + " as (H, W)")


def test_colorize_with_given_bounds_masks_and_values_that_are_not_finite():
    z = np.load(GOLDEN)
    table, lut = z["lut"], _lut()
    value = z["in_m17x300_block"].copy()
    value[0, 0, :4] = [np.inf, -np.inf, np.nan, 0.0]
    vd = _dev(value)
    for kw in (dict(vmin=0.5, vmax=4.0), dict(vmin=0.1), dict(vmax=3.3), dict(vmin=2.0, vmax=2.0), dict(vmin=4.0, vmax=0.5), dict(vmin=0.5, vmax=4.0, invalid_val=None),
               dict(vmin=1 / 3, vmax=10 / 3, background=(1, 2, 3)), dict(background=(255, 0, 7), invalid_val=0.0)):
        want, status = ref.colorize(value, table, **kw)
        got, st = fe.colorize(vd, lut, return_status=True, **kw)
        _same(got, want, "colorize %r" % (kw,))
        assert int(st) == status == 0
    assert (ref.colorize(value, table, vmin=2.0, vmax=2.0)[0][0, 0] == 0).all()          # inf * 0 is NaN: matplotlib's `bad` colour
    rng = np.random.default_rng(3)
    for mask in (rng.random(value.shape[1:]) < 0.3, (rng.random(value.shape) < 0.5).astype(np.uint8), (rng.random(value.shape[1:]) < 0.1).astype(np.int64) * 7):
        want, _ = ref.colorize(value, table, invalid_mask=mask)
        _same(fe.colorize(vd, lut, invalid_mask=_dev(mask)), want, "colorize with a %s mask" % mask.dtype)
        assert (want[4, 100] != 128).any() or mask.reshape(value.shape[1:])[4, 100]          # with a mask, -99 is a depth like any other
    # nothing valid: background everywhere, status bit 1
    got, st = fe.colorize(torch.full((1, 5, 7), -99.0, device=DEV), lut, return_status=True)
    assert int(st) == ref.NO_VALID and (got.cpu().numpy() == 128).all()


@functools.lru_cache(maxsize=None)
def _full_hd():
    v = ref.depth_values(1080 * 1920, ties=True).reshape(1, 1080, 1920)
    z = np.load(GOLDEN)
    return v, ref.percentile(v, (2, 85))[0], ref.colorize(v, z["lut"])[0]


def test_full_hd_percentiles_and_colours():
    """The one size at which float32 (n - 1) q has a coarse fraction, the histograms span the whole capped grid and a third of the keys share one bin."""
    v, want_p, want_img = _full_hd()
    assert (v == 0).sum() == 691200
    vd = _dev(v)
    _same_bits(fe.percentile(vd, (2, 85)), want_p, "1080p percentiles")
    _same_bits(fe.percentile(vd, (0, 33.4, 50, 100)), ref.percentile(v, (0, 33.4, 50, 100))[0], "1080p, four percentiles")
    a = fe.colorize(vd, _lut())
    _same(a, want_img, "1080p colorize")
    assert torch.equal(fe.colorize(vd, _lut()), a)


# ---- rule 6 ----------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _package(h=33, w=65):
    render, gt, pred = (ref.rule_inputs(h, w, seed=s) for s in (0, 2, 4))
    normal = (ref.rule_inputs(h, w, seed=1) * np.float32(2) - np.float32(1)).astype(np.float32)
    residual = _residual(ref.rule_inputs(h, w, seed=3))
    depth = ref.depth_values(h * w, seed=6).reshape(1, h, w)
    depth[0, 3:9, 10:46] = -99
    host = dict(render=render, gt=gt, image_pred=pred, normal=normal, residual=residual, depth=depth)
    return host, {k: _dev(v) for k, v in host.items()}


def _export(d, split, with_fusion=True, with_gt=True):
    pkg = dict(render=d["render"], median_intersected_depth=d["depth"], rendered_normal=d["normal"])
    return fe.export_frame(pkg, dict(image_pred=d["image_pred"], residual=d["residual"]) if with_fusion else None, d["gt"] if with_gt else None, _lut(), split)


@pytest.mark.parametrize("split", ["test", "train"])
def test_export_frame_is_the_single_rules_in_one_buffer(split):
    host, d = _package()
    lut_host = np.load(GOLDEN)["lut"]
    frame = _export(d, split)
    want, status = ref.export_frame(host["render"], host["depth"], host["normal"], lut_host, host["gt"], host["image_pred"], host["residual"], split)
    assert sorted(frame) == sorted(list(want) + ["packed", "status", "layout"]) and sorted(want) == ["aggregate", "depth", "gt", "normal", "render", "residual"]
    single = {"render": fe.to_u8(d["render"]) if split == "test" else fe.to_u8(d["render"], "truncate", "bgr"), "gt": fe.to_u8(d["gt"]), "aggregate": fe.to_u8(d["image_pred"]),
              "residual": fe.residual_vis_u8(d["residual"])[0], "depth": fe.colorize(d["depth"], _lut()), "normal": fe.normal_to_u8(d["normal"])}
    packed = frame["packed"]
    assert packed.dtype == torch.uint8 and packed.dim() == 1 and packed.is_contiguous() and int(frame["status"]) == status == 0
    for key, img in want.items():
        view = frame[key]
        _same(view, img, "%s (%s)" % (key, split))
        assert torch.equal(view, single[key]), key
        offset = frame["layout"][key][0]
        assert view.dtype == torch.uint8 and tuple(view.shape) == (33, 65, 3) and view.is_contiguous() and view.data_ptr() == packed.data_ptr() + offset and offset % 4 == 0
        assert view.untyped_storage().data_ptr() == packed.untyped_storage().data_ptr()
    assert frame["status"].data_ptr() == packed.data_ptr() + frame["layout"]["status"][0]
    # the one copy
    on_host = fe.to_host(frame)
    assert sorted(on_host) == sorted(list(want) + ["status"]) and on_host["status"] == 0
    for key, img in want.items():
        assert isinstance(on_host[key], np.ndarray) and np.array_equal(on_host[key], img), key
    mine = torch.empty(packed.numel() + 100, dtype=torch.uint8, pin_memory=True)
    again = fe.to_host(frame, pinned=mine)
    assert all(np.array_equal(again[k], want[k]) for k in want) and np.shares_memory(again["render"], mine.numpy())
    # two runs: the same bytes, the bytes between the images included
    assert torch.equal(_export(d, split)["packed"], packed)
    # fewer images: fewer views, the same bytes in each
    small = _export(d, split, with_fusion=False, with_gt=False)
    assert sorted(small) == ["depth", "layout", "normal", "packed", "render", "status"] and all(torch.equal(small[k], frame[k]) for k in ("depth", "normal", "render"))


def test_export_frame_status_bits():
    _, d = _package()
    flat = dict(d, residual=torch.zeros_like(d["residual"]), depth=torch.full_like(d["depth"], -99.0))
    frame = _export(flat, "test")
    assert int(frame["status"]) == ref.ZERO_RESIDUAL | ref.NO_VALID and fe.to_host(frame)["status"] == 3
    assert int(frame["residual"].max()) == 0 and bool((frame["depth"] == 128).all()) and torch.equal(frame["render"], _export(d, "test")["render"])


# ---- dirty, guard-banded buffers -------------------------------------------------------------------------------------------------------------------------
def test_on_dirty_guard_banded_buffers():
    """Every output and the arena served from blocks of 0x00, 0xFF and 0x40 between guards (tests/dirty_alloc.py): the same bytes, the guards untouched.  The
    counts are the wrapper's allocations: the image, the status word, and the arena where a select or a residual needs one."""
    host, d = _package()
    lut_host = np.load(GOLDEN)["lut"]
    x13 = _dev(ref.rule_inputs(1, 3))
    base = dict(da.check("to_u8 1x3", lambda: fe.to_u8(x13), DEV, 2))
    _same(base["result"], ref.to_u8(ref.rule_inputs(1, 3)), "to_u8 on dirty buffers")
    base = dict(da.check("normal_to_u8 33x65", lambda: fe.normal_to_u8(d["normal"]), DEV, 2))
    _same(base["result"], ref.normal_to_u8(host["normal"]), "normal_to_u8 on dirty buffers")
    base = dict(da.check("residual_vis_u8 33x65", lambda: fe.residual_vis_u8(d["residual"]), DEV, 3))
    _same(base["[0]"], ref.residual_vis_u8(host["residual"])[0], "residual_vis_u8 on dirty buffers")
    for name in ("n2145", "both_zeros", "val_and_mask", "all_invalid"):
        _, v, qs, inv, mask = CASES[name]
        vd, md = _dev(v), None if mask is None else _dev(mask)
        base = dict(da.check("percentile " + name, lambda: fe.percentile(vd, qs, inv, md, return_status=True), DEV, 3))
        _same_bits(base["[0]"], ref.percentile(v, qs, inv, mask)[0], name + " on dirty buffers")
    base = dict(da.check("colorize 33x65", lambda: fe.colorize(d["depth"], _lut(), return_status=True), DEV, 3))
    _same(base["[0]"], ref.colorize(host["depth"], lut_host)[0], "colorize on dirty buffers")
    base = dict(da.check("quantize 33x65", lambda: fe.quantize(d["render"]), DEV, 1))
    for split in ("test", "train"):
        def call():
            frame = _export(d, split)
            frame.pop("layout")          # (offsets and shapes: not tensors)
            return frame
        base = dict(da.check("export_frame 33x65 " + split, call, DEV, 2))
        want, _ = ref.export_frame(host["render"], host["depth"], host["normal"], lut_host, host["gt"], host["image_pred"], host["residual"], split)
        for key, img in want.items():
            _same(base["[%r]" % key], img, key + " on dirty buffers")
        assert int(base["['status']"]) == 0


# ---- rule 7 ----------------------------------------------------------------------------------------------------------------------------------------------
def _parent_image_metrics(renders, gts):
    """image_eval.image_metrics as it stood before the keyword, line by line"""
    dims = losses._ssim_check("image_metrics", renders, gts, 11, (3, 4))
    x = renders.detach().float().contiguous()
    y = gts.detach().float().contiguous()
    n = dims[0]
    with torch.cuda.device(x.device):
        per, mse, l1 = (torch.empty(n, dtype=torch.float32, device=x.device) for _ in range(3))
    losses._ssim_forward(dims, x, y, per_image=per, mse=mse, l1_per_image=l1)
    return {"ssim": per, "psnr": 20.0 * torch.log10(1.0 / torch.sqrt(mse)), "l1": l1}


def test_quantized_metrics_are_the_metrics_of_the_quantised_images():
    rng = np.random.default_rng(11)
    x = np.clip(np.stack([ref.rule_inputs(32, 48, seed=s) for s in (0, 1)]), -0.2, 1.2)          # (without the 1e30s: the unquantised SSIM must be a number)
    y =np.clip(x + rng.normal(0, 0.05, x.shape), -0.1, 1.1).astype(np.float32)
    xd, yd = _dev(x), _dev(y)
    got = image_eval.image_metrics(xd, yd, quantize=True)
    want = image_eval.image_metrics(_dev(ref.quantize(x)), _dev(ref.quantize(y)))
    plain = image_eval.image_metrics(xd, yd)
    parent = _parent_image_metrics(xd, yd)
    assert sorted(got) == sorted(want) == sorted(plain) == sorted(parent) == ["l1", "psnr", "ssim"]
    for k in got:
        assert torch.equal(got[k], want[k]) and torch.equal(plain[k], parent[k]) and torch.equal(image_eval.image_metrics(xd, yd, quantize=False)[k], parent[k]), k
        assert not torch.equal(got[k], plain[k]), k          # the quantisation is visible in every number
    # evaluate_images: the same numbers through the list form
    ev = image_eval.evaluate_images([xd[0], xd[1]], [yd[0], yd[1]], quantize=True)
    assert ev["per_view"]["SSIM"]["00001"] == float(want["ssim"][1]) and ev["per_view"]["PSNR"]["00000"] == float(want["psnr"][0])
    ev0 = image_eval.evaluate_images([xd[0], xd[1]], [yd[0], yd[1]])
    assert ev0["per_view"]["SSIM"]["00001"] == float(parent["ssim"][1]) and ev0["PSNR"] != ev["PSNR"]
