"""TSDF fusion of rendered depth maps and marching-cubes mesh extraction on the MI355X: the mesh output of the reference's `render.py --render_geo`
(render.py:228-286, 328-331, 355-364), which runs Open3D's host-side `ScalableTSDFVolume` and cannot be produced where Open3D has no build.

    volume = TSDFVolume(voxel_length=voxel_size, sdf_trunc=4 * voxel_size)
    for view in views:
        out = renderer.render(view, ...)
        volume.integrate_view(view, depth_for_fusion(out, view, max_depth, use_depth_filter, bounds), color=out["render"])
    raw = volume.extract_mesh()
    ply.save_mesh(path, raw)                                                   # tsdf_fusion.ply
    ply.save_mesh(path_post, mesh.post_process_mesh(raw, num_cluster))         # tsdf_fusion_post.ply (ibgs_amd/mesh.py: the largest clusters only)

The contract (block layout, per-voxel update in its f32 operation order, marching cubes) is this project's own statement of the legacy Open3D volume:
DESIGN.md section 11 and the header of ibgs_amd/csrc/tsdf.hip; tests/tsdf_ref.py restates it in numpy.

HIP only (C ABI include/ibgs_tsdf.h): CPU tensors are refused, every kernel runs on torch's current stream.  `integrate` never waits for the device;
`check()` and `extract_mesh()` read the volume's counters back."""
import ctypes
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _device, _lib

BLOCK = 8
VOXELS = BLOCK ** 3
KEY_BITS = 21
KEY_BIAS = 1 << (KEY_BITS - 1)
INT64_MAX = (1 << 63) - 1
# default block capacity: this share of the device memory free at first use, under a ceiling (rasterizer._cache_cap decides it once per device)
CAPACITY_FRACTION = 0.1
CAPACITY_CEILING_BYTES = 16 << 30
# device bytes per block of capacity: voxels (5 f32 each) + block key + two hash slots (key, block, mark, active entry) + mesh scratch
BYTES_PER_BLOCK = VOXELS * 20 + 8 + 2 * (8 + 4 + 4 + 4) + VOXELS * 2 + 8 + 4 + 8


class TriangleMesh(NamedTuple):
    vertices: torch.Tensor          # (V, 3) f32
    faces: torch.Tensor             # (F, 3) int32, each row oriented towards increasing tsdf (free space)
    colors: torch.Tensor            # (V, 3) f32
    normals: torch.Tensor           # (V, 3) f32, unit (or zero)


class TSDFVolumeError(RuntimeError):
    pass


def pack_keys(coords):
    """(N, 3) integer block coordinates -> (N,) int64 packed keys x | y << 21 | z << 42 (each biased by 2^20)."""
    c = np.asarray(coords, np.int64) + KEY_BIAS
    return c[:, 0] | (c[:, 1] << KEY_BITS) | (c[:, 2] << (2 * KEY_BITS))


def unpack_keys(keys):
    k = np.asarray(keys, np.int64)
    m = (1 << KEY_BITS) - 1
    return np.stack([k & m, (k >> KEY_BITS) & m, (k >> (2 * KEY_BITS)) & m], axis=1) - KEY_BIAS


def pose_inverse(world_to_camera):
    """camera_to_world as the library receives it: the float64 inverse of the f32 pose, rounded to f32 (tests/tsdf_ref.py uses the same)."""
    return np.linalg.inv(np.asarray(world_to_camera, np.float32).astype(np.float64)).astype(np.float32)


def _host_pose(world_to_camera):
    if torch.is_tensor(world_to_camera):
        world_to_camera = world_to_camera.detach().cpu().numpy()          # (a device tensor is read back: pass host poses to stay asynchronous)
    m = np.asarray(world_to_camera, dtype=np.float64)
    if m.shape != (4, 4):
        raise ValueError("world_to_camera must be 4 x 4, got %s" % (m.shape,))
    if not np.all(np.isfinite(m)):
        raise ValueError("world_to_camera is not finite")
    m32 = m.astype(np.float32)
    inv = pose_inverse(m32)
    if not np.all(np.isfinite(inv)):
        raise ValueError("world_to_camera is singular")
    return m32, inv


class TSDFVolume:
    """Sparse TSDF volume of 8^3-voxel blocks (Open3D's ScalableTSDFVolume with color_type RGB8, as render.py builds it)."""

    def __init__(self, voxel_length, sdf_trunc, block_capacity=None, device=None):
        voxel_length, sdf_trunc = float(voxel_length), float(sdf_trunc)
        if not (math.isfinite(voxel_length) and voxel_length > 0 and math.isfinite(sdf_trunc) and sdf_trunc > 0):
            raise ValueError("voxel_length and sdf_trunc must be finite and > 0")
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("ibgs_amd.tsdf runs on the MI355X only (no CPU path)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if block_capacity is None:
            from .rasterizer import _cache_cap
            block_capacity = max(1, _cache_cap(device, None, CAPACITY_CEILING_BYTES, CAPACITY_FRACTION) // BYTES_PER_BLOCK)
        block_capacity = int(block_capacity)
        if not 1 <= block_capacity <= (1 << 29):
            raise ValueError("block_capacity must be in [1, 2^29], got %d" % block_capacity)
        self.voxel_length, self.sdf_trunc, self.capacity, self.device = voxel_length, sdf_trunc, block_capacity, device
        self.slot_bits = max(1, (2 * block_capacity - 1).bit_length())          # >= 2 x capacity slots: short probe chains
        self._lib = _lib.load()
        S = 1 << self.slot_bits
        with torch.cuda.device(device):
            self._slot_key = torch.empty(S, dtype=torch.int64, device=device)
            self._slot_block = torch.empty(S, dtype=torch.int32, device=device)
            self._slot_mark = torch.empty(S, dtype=torch.int32, device=device)
            self._active = torch.empty(S, dtype=torch.int32, device=device)
            self._block_key = torch.empty(block_capacity, dtype=torch.int64, device=device)
            self._vox = torch.empty(5, block_capacity, VOXELS, dtype=torch.float32, device=device)          # tsdf, weight, colour r g b
            self._state = torch.empty(_lib.TSDF_STATE_WORDS, dtype=torch.int32, device=device)
        self._mc = None
        self.reset()

    # -- plumbing ---------------------------------------------------------------------------------------------------------------------------
    def _vol(self):
        v = _lib.TsdfVolume()
        v.voxel_length, v.sdf_trunc, v.capacity, v.slot_bits = self.voxel_length, self.sdf_trunc, self.capacity, self.slot_bits
        v.slot_key, v.slot_block, v.slot_mark, v.active = (t.data_ptr() for t in (self._slot_key, self._slot_block, self._slot_mark, self._active))
        v.block_key, v.state = self._block_key.data_ptr(), self._state.data_ptr()
        v.tsdf, v.weight, v.color = self._vox[0].data_ptr(), self._vox[1].data_ptr(), self._vox[2].data_ptr()
        return v

    def _counters(self):
        s = self._state.cpu().tolist()          # (waits for the stream)
        return {"allocated": s[_lib.TSDF_ALLOCATED], "failed": s[_lib.TSDF_FAILED], "ignored": s[_lib.TSDF_IGNORED],
                "vertices": s[_lib.TSDF_VERTICES], "faces": s[_lib.TSDF_FACES], "overrun": s[_lib.TSDF_OVERRUN], "table_full": s[_lib.TSDF_TABLE_FULL]}

    def _raise_if_failed(self, c):
        if c["failed"] or c["table_full"]:
            raise TSDFVolumeError("TSDF volume overflow: %s%d block(s) found no room (capacity %d blocks%s); the volume is unusable until reset()"
                                  % ("at least " if c["table_full"] else "", c["failed"], self.capacity,
                                     ", and the hash table filled up" if c["table_full"] else ""))

    # -- public -----------------------------------------------------------------------------------------------------------------------------
    def reset(self):
        """Empty the volume (and clear an overflow)."""
        with torch.cuda.device(self.device):
            self._slot_key.fill_(-1); self._slot_block.fill_(-1); self._slot_mark.zero_(); self._active.zero_()
            self._block_key.fill_(INT64_MAX); self._vox.zero_(); self._state.zero_()

    def check(self):
        """Raise if a block found no room since the last reset() (reads the counters back)."""
        self._raise_if_failed(self._counters())

    def num_blocks(self):
        c = self._counters()
        return min(c["allocated"], self.capacity)

    def ignored_points(self):
        """Valid pixels whose truncation cube left the packable block range (they were skipped)."""
        return self._counters()["ignored"]

    def integrate(self, depth, fx, fy, cx, cy, world_to_camera, color=None, depth_trunc=math.inf, dedup=True):
        """Fuse one view.  depth (H, W) f32 on the device, 0 = none; color (3, H, W) f32 or None (colours left as they are); pixel centres at
        integer coordinates; world_to_camera 4 x 4 (a host array keeps the call free of any wait on the device).  `dedup=False` sends every
        (pixel, block) pair to the global hash (A/B measurements only)."""
        if not torch.is_tensor(depth) or not depth.is_cuda:
            raise RuntimeError("TSDFVolume.integrate runs on the MI355X only (depth must be a device tensor)")
        if depth.dim() == 3 and depth.shape[0] == 1:
            depth = depth[0]
        if depth.dim() != 2 or depth.dtype != torch.float32:
            raise ValueError("depth must be (H, W) float32, got %s %s" % (tuple(depth.shape), depth.dtype))
        if depth.device != self.device:
            raise ValueError("depth is on %s, the volume on %s" % (depth.device, self.device))
        H, W = int(depth.shape[0]), int(depth.shape[1])
        if color is not None:
            if not torch.is_tensor(color) or not color.is_cuda:
                raise RuntimeError("TSDFVolume.integrate: color must be a device tensor")
            if tuple(color.shape) != (3, H, W) or color.dtype != torch.float32 or color.device != self.device:
                raise ValueError("color must be (3, %d, %d) float32 on %s, got %s %s" % (H, W, self.device, tuple(color.shape), color.dtype))
        k = [float(x) for x in (fx, fy, cx, cy)]
        if not all(math.isfinite(x) for x in k) or k[0] == 0 or k[1] == 0:
            raise ValueError("intrinsics must be finite with fx, fy != 0")
        depth_trunc = float(depth_trunc)
        if math.isnan(depth_trunc):
            raise ValueError("depth_trunc is NaN")
        w2c, c2w = _host_pose(world_to_camera)
        view = _lib.TsdfView()
        view.W, view.H = W, H
        view.fx, view.fy, view.cx, view.cy = k
        view.depth_trunc = depth_trunc
        view.world_to_camera[:] = [float(x) for x in w2c[:3].reshape(-1)]
        view.camera_to_world[:] = [float(x) for x in c2w[:3].reshape(-1)]
        d = depth.contiguous()
        c = None if color is None else color.contiguous()
        _device.call(self.device, "ibgs_tsdf_integrate", ctypes.byref(self._vol()), ctypes.byref(view), d.data_ptr(), None if c is None else c.data_ptr(),
                     0 if dedup else _lib.TSDF_FLAG_NO_DEDUP)

    def integrate_view(self, camera, depth, color=None, depth_trunc=math.inf):
        """integrate() with the intrinsics Fx, Fy, Cx, Cy of a reference `Camera` (or simple_scene.SimpleCamera) and the pose render.py:275-277
        builds: [R^T | T] from the camera's host-side R and T (that is world_view_transform.T; used when R / T are missing)."""
        R, T = getattr(camera, "R", None), getattr(camera, "T", None)
        if R is not None and T is not None and not (torch.is_tensor(R) and R.is_cuda) and not (torch.is_tensor(T) and T.is_cuda):
            pose = np.identity(4)
            pose[:3, :3] = np.asarray(R.detach().cpu() if torch.is_tensor(R) else R, np.float64).T
            pose[:3, 3] = np.asarray(T.detach().cpu() if torch.is_tensor(T) else T, np.float64)
        else:
            pose = camera.world_view_transform.T
        self.integrate(depth, camera.Fx, camera.Fy, camera.Cx, camera.Cy, pose, color=color, depth_trunc=depth_trunc)

    def _mesh_scratch(self):
        if self._mc is None:
            with torch.cuda.device(self.device):
                self._mc = {"rank": torch.empty(self.capacity, dtype=torch.int32, device=self.device),
                            "vinfo": torch.empty(self.capacity * VOXELS, dtype=torch.int16, device=self.device),
                            "vcount": torch.empty(self.capacity + 1, dtype=torch.int32, device=self.device),
                            "fcount": torch.empty(self.capacity + 1, dtype=torch.int32, device=self.device)}
        return self._mc

    def extract_mesh(self):
        """Marching cubes over every cell whose 8 voxels have weight > 0 -> TriangleMesh on the device (one vertex per crossing edge, no
        unreferenced vertices, fixed order: equal volumes give bit-identical meshes).  Raises if the volume overflowed."""
        mc = self._mesh_scratch()
        with torch.cuda.device(self.device):
            order = torch.sort(self._block_key).indices          # blocks by ascending key; free blocks (INT64_MAX) last
            sc = _lib.TsdfMeshScratch()
            sc.order, sc.rank, sc.vinfo, sc.vcount, sc.fcount = (order.data_ptr(), mc["rank"].data_ptr(), mc["vinfo"].data_ptr(),
                                                                 mc["vcount"].data_ptr(), mc["fcount"].data_ptr())
            vol = self._vol()
            _device.call(self.device, "ibgs_tsdf_mesh_count", ctypes.byref(vol), ctypes.byref(sc))
            c = self._counters()          # the one read-back: overflow, and the totals that size the outputs
            self._raise_if_failed(c)
            V, F = c["vertices"], c["faces"]
            vert = torch.empty(V, 3, dtype=torch.float32, device=self.device)
            nrm = torch.empty(V, 3, dtype=torch.float32, device=self.device)
            col = torch.empty(V, 3, dtype=torch.float32, device=self.device)
            faces = torch.empty(F, 3, dtype=torch.int32, device=self.device)
            _device.call(self.device, "ibgs_tsdf_mesh_emit", ctypes.byref(vol), ctypes.byref(sc), V, F, vert.data_ptr(), nrm.data_ptr(), col.data_ptr(),
                         faces.data_ptr())
        return TriangleMesh(vert, faces, col, nrm)

    def mesh_overruns(self):
        """Emits that fell outside the output arrays in extract_mesh() (always 0 unless the library is broken; the tests check it)."""
        return self._counters()["overrun"]

    def blocks(self):
        """The allocated blocks in ascending key order: {"keys" (N,) int64 packed, "coords" (N, 3) int64 block coordinates, "tsdf" (N, 512),
        "weight" (N, 512), "color" (N, 512, 3)} as numpy arrays; voxel l = i + 8 j + 64 k of block (bx, by, bz) is voxel (8 bx + i, ...)."""
        n = self.num_blocks()
        keys = self._block_key[:n].cpu().numpy()
        order = np.argsort(keys, kind="stable")
        vox = self._vox[:, :n].cpu().numpy()[:, order]
        keys = keys[order]
        return {"keys": keys, "coords": unpack_keys(keys), "tsdf": vox[0], "weight": vox[1], "color": np.ascontiguousarray(vox[2:].transpose(1, 2, 0))}


def camera_rays(camera, device=None):
    """Camera.get_rays() (scene/cameras.py:120-128, scale 1): (H, W, 3) rays ((u - Cx) / Fx, (v - Cy) / Fy, 1) at integer pixel centres."""
    W, H = int(camera.image_width), int(camera.image_height)
    ix, iy = torch.meshgrid(torch.arange(W), torch.arange(H), indexing="xy")
    rays = torch.stack([(ix - camera.Cx) / camera.Fx * 1.0, (iy - camera.Cy) / camera.Fy * 1.0, torch.ones_like(ix)], -1).float()
    return rays if device is None else rays.to(device)


def depth_for_fusion(render_pkg, camera, max_depth, use_depth_filter=False, bounds=None):
    """The depth map render.py fuses for one view (render.py:228-286), as an (H, W) f32 tensor on the depth's device, 0 = not fused:

      - the median depth `render_pkg["median_intersected_depth"]` (render.py's DEFAULT_DEPTH_TYPE);
      - use_depth_filter: 0 where the angle between normalize(get_rays()) and the normalised depth normal exceeds 80 degrees (render.py:251-258).
        render.py renders with return_depth_normal=False and then reads that normal, which is None there (a bug of the reference: the filter
        cannot run).  Here a missing normal is computed from the depth (depthnormal.depth_normal, what render() returns with
        return_depth_normal=True);
      - bounds (3, 2) [min, max] per axis: 0 where the back-projected point (GaussianModel.get_points_from_depth) leaves the box (render.py:266-272);
      - max_depth: 0 beyond it (Open3D's depth_trunc, render.py:281-282)."""
    depth = render_pkg["median_intersected_depth"].detach().squeeze().float().clone()
    H, W = depth.shape
    dev = depth.device
    if use_depth_filter:
        view_dir = torch.nn.functional.normalize(camera_rays(camera, dev), p=2, dim=-1)
        dn = render_pkg.get("median_intersected_depth_normal")
        if dn is None:
            from .depthnormal import depth_normal
            dn = depth_normal(camera, depth)
        dn = torch.nn.functional.normalize(dn.detach().permute(1, 2, 0), p=2, dim=-1)
        dot = torch.sum(view_dir * dn, dim=-1).abs()
        angle = torch.acos(dot)
        depth[angle > (80.0 / 180 * 3.14159)] = 0
    if bounds is not None:
        b = torch.as_tensor(np.asarray(bounds, np.float32), device=dev)
        pts = (camera_rays(camera, dev) * depth[..., None]).reshape(-1, 3)
        R = torch.as_tensor(np.asarray(camera.R.detach().cpu() if torch.is_tensor(camera.R) else camera.R), dtype=torch.float32, device=dev)
        T = torch.as_tensor(np.asarray(camera.T.detach().cpu() if torch.is_tensor(camera.T) else camera.T), dtype=torch.float32, device=dev)
        pts = (pts - T) @ R.transpose(-1, -2)
        bad = ((pts[..., 0] < b[0, 0]) | (pts[..., 0] > b[0, 1]) | (pts[..., 1] < b[1, 0]) | (pts[..., 1] > b[1, 1])
               | (pts[..., 2] < b[2, 0]) | (pts[..., 2] > b[2, 1]))
        depth[bad.reshape(H, W)] = 0
    depth[depth > float(max_depth)] = 0
    return depth
