"""Training targets from a fitted body mesh and object mesh, computed on the GPU.

`BoundarySampler` keeps the contract of the reference's class of the same name (preprocess/boundary_sampler.py, driven by
preprocess/preprocess_scale.py): method names, argument lists, return order, dictionary keys, dtypes and shapes.  The work
behind it is this package's: surface samples, Gaussian offsets and grid points are drawn on the device from a
`torch.Generator`, the distances to the two meshes, the closest points and the nearest body vertex (whose part label is the
point's label) come from `mesh_distance` (csrc/mesh_dist.hip) -- no igl, trimesh or psbody.  A mesh is any object with
`.v` / `.f` or `.vertices` / `.faces`.

Difference from the reference, on purpose: the random numbers come from the sampler's own generator (`seed`), not from
numpy's global stream; the distributions are the same (area-weighted triangle of the COMBINED mesh and a uniform barycentric
point, + sigma N(0,1); grid points uniform in `get_bounds()`).

`train_batch` is an addition: the targets of one training step under `CHORE.forward`'s keyword names, drawn directly from
meshes on the device.
"""
import os
from types import SimpleNamespace

import numpy as np
import torch

from .mesh_distance import mesh_distance

FLIP_PARTS = {1: 6, 2: 7, 3: 8, 4: 9, 5: 10, 12: 13, 6: 1, 7: 2, 8: 3, 9: 4, 10: 5, 13: 12}      # left <-> right


def _arrays(mesh):
    """(vertices (V,3) float64, faces (F,3) int64) of a psbody-style (.v/.f) or trimesh-style (.vertices/.faces) mesh"""
    if isinstance(mesh, _DeviceMesh):
        return mesh.v, mesh.f
    v = mesh.v if hasattr(mesh, "v") else mesh.vertices
    f = mesh.f if hasattr(mesh, "f") else mesh.faces
    return np.asarray(v, np.float64), np.asarray(f).astype(np.int64)


class _DeviceMesh:
    """a mesh and its copy on the device (made once per boundary_sample_all call)"""

    def __init__(self, mesh, device):
        self.v, self.f = _arrays(mesh)
        self.vertices, self.faces = self.v, self.f
        self.vt = torch.as_tensor(np.ascontiguousarray(self.v, np.float32)).to(device)
        self.ft = torch.as_tensor(np.ascontiguousarray(self.f, np.int32)).to(device)


def sample_surface(verts, faces, count, generator=None):
    """`count` uniform points on the surface: verts (V,3) or (B,V,3) float32 and faces (F,3) on the device -> (points
    (count,3) or (B,count,3), face (count,) or (B,count) int64 index of the triangle each point was drawn on).  The device form
    of recon_fit_base.sample_surface: area-weighted triangle, uniform barycentric point."""
    unbatched = verts.dim() == 2
    v = verts[None] if unbatched else verts
    f = faces.long()
    tri = v[:, f]                                                     # (B,F,3,3)
    e1, e2 = tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0]
    area = torch.linalg.cross(e1, e2).double().norm(dim=-1)          # twice the area: the weights' scale does not matter
    cum = torch.cumsum(area, 1)
    B = v.shape[0]
    r = torch.rand((B, count, 3), device=v.device, dtype=torch.float64, generator=generator)
    idx = torch.searchsorted(cum, r[:, :, 0] * cum[:, -1:]).clamp_(max=f.shape[0] - 1)
    a, b = r[:, :, 1].float(), r[:, :, 2].float()
    flip = a + b > 1
    a, b = torch.where(flip, 1 - a, a), torch.where(flip, 1 - b, b)
    bi = torch.arange(B, device=v.device)[:, None]
    pts = tri[bi, idx, 0] + a[..., None] * e1[bi, idx] + b[..., None] * e2[bi, idx]
    return (pts[0], idx[0]) if unbatched else (pts, idx)


class BoundarySampler:
    def __init__(self, *, device="cuda:0", part_labels=None, seed=None):
        """device: where the work runs; part_labels: (6890,) label of every SMPL vertex (default: the table FileAssets reads
        from smpl_parts_dense.pkl under PATHS.yml's SMPL_ASSETS_ROOT, or under ./assets like the reference, read on first
        use); seed: of the sampler's torch.Generator (default: a fresh random seed)"""
        self.device = torch.device(device)
        self._labels = None if part_labels is None else np.asarray(part_labels, np.int32)
        self._labels_dev = None
        self.seed = seed
        self._gen = None

    # ---- state ----------------------------------------------------------------------------------------------------
    @property
    def generator(self):
        if self._gen is None:
            self._gen = torch.Generator(device=self.device)
            if self.seed is None:
                self._gen.seed()
            else:
                self._gen.manual_seed(int(self.seed))
        return self._gen

    @property
    def part_labels(self):
        if self._labels is None:
            from ..recon.assets import FileAssets
            fa = FileAssets.from_paths_yml() if os.path.isfile("PATHS.yml") else FileAssets("assets")
            self._labels = np.asarray(fa.part_labels(), np.int32)
        return self._labels

    def _labels_on_device(self):
        if self._labels_dev is None:
            self._labels_dev = torch.as_tensor(self.part_labels.astype(np.int64)).to(self.device)
        return self._labels_dev

    # ---- the reference's methods -------------------------------------------------------------------------------------
    def boundary_sampling(self, smpl, obj, sigma=0.05, sample_num=100000, grid_ratio=0.01, points=None):
        """-> (samples_all (n,3) float64, d_h (n,) float32, d_o (n,) float32, parts (n,) int32, neighbours_h (n,3) float32,
        neighbours_o (n,3) float32) with n = sample_num + int(grid_ratio * sample_num): surface samples of the combined
        mesh + sigma N(0,1), then grid points.  `points` (n,3): these samples are labelled instead (nothing is drawn)."""
        smpl, obj = self._on_device(smpl), self._on_device(obj)
        if points is None:
            pts = self._draw(smpl.vt[None], smpl.ft, obj.vt[None], obj.ft, sigma, sample_num, int(grid_ratio * sample_num),
                             self.generator)[0]
        else:
            pts = torch.as_tensor(np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))).to(self.device)
        d_h, near_h, vid = mesh_distance(pts, smpl.vt, smpl.ft, ("dist", "closest", "vert_idx"))
        d_o, near_o = mesh_distance(pts, obj.vt, obj.ft, ("dist", "closest"))
        # one download: the vertex index is exact in float32 (V < 2^24)
        host = torch.cat([pts, d_h[:, None], d_o[:, None], vid[:, None].float(), near_h, near_o], 1).cpu().numpy()
        parts = self.part_labels[host[:, 5].astype(np.int64)]
        return (host[:, 0:3].astype(np.float64), host[:, 3].copy(), host[:, 4].copy(), parts, host[:, 6:9].copy(),
                host[:, 9:12].copy())

    def flip_part_labels(self, parts):
        "left and right body part labels swapped, the others kept"
        parts = np.asarray(parts)
        new_labels = parts.copy()
        for src, dst in FLIP_PARTS.items():
            new_labels[parts == src] = dst
        return new_labels

    def get_sample_num(self, ratio, total_sample, thres=10000):
        return max(int(ratio * total_sample), thres)

    def boundary_sample_all(self, landmark, smpl_mesh, obj_mesh, sigmas, ratios, sample_num, grid_ratio=1 / 16., flip=False):
        """the dictionary preprocess_scale.py saves for one frame and camera: `points`, `dist_h`, `dist_o`, `parts` as
        dictionaries keyed 'sigma{s}' (float32, float32, float32, uint8), `pca_axis` float32 (3,3), `smpl_center`,
        `body_kpts` float32 (25,3), `obj_center` float32 (3,)"""
        smpl, obj = self._on_device(smpl_mesh), self._on_device(obj_mesh)
        points_all, dh_all, do_all, parts_all = {}, {}, {}, {}
        for s, r in zip(sigmas, ratios):
            n = self.get_sample_num(r, sample_num)
            points, d_h, d_o, parts, _, _ = self.boundary_sampling(smpl, obj, s, n, grid_ratio=grid_ratio)
            key = "sigma{}".format(s)
            points_all[key] = points.astype(np.float32)
            dh_all[key] = d_h.astype(np.float32)
            do_all[key] = d_o.astype(np.float32)
            parts_all[key] = (self.flip_part_labels(parts) if flip else parts).astype(np.uint8)
        return {
            "points": points_all,
            "dist_h": dh_all,
            "dist_o": do_all,
            "parts": parts_all,
            "pca_axis": BoundarySampler.compute_pca(obj).astype(np.float32),
            "smpl_center": landmark.get_smpl_center(smpl_mesh),
            "body_kpts": np.asarray(landmark.get_body_kpts(smpl_mesh)).astype(np.float32),
            "obj_center": np.mean(obj.v, 0).astype(np.float32),
        }

    @staticmethod
    def compute_pca(obj):
        "PCA axes (3,3) of the object's vertices: sklearn's, whose sign convention is part of the training target"
        from sklearn.decomposition import PCA
        pca = PCA(n_components=3)
        pca.fit(np.asarray(obj.v if hasattr(obj, "v") else obj.vertices, np.float64))
        return pca.components_

    def get_grid_samples(self, pmin, pmax, sample_num):
        "sample_num uniform points in the box [pmin, pmax] -> (sample_num, 3) float64"
        return self._grid(np.asarray(pmin), np.asarray(pmax), (sample_num,), self.generator).double().cpu().numpy()

    @staticmethod
    def get_bounds():
        "the fixed box of the grid points, in camera coordinates (metres)"
        return np.array([-3.0, -0.9, 0.2]), np.array([3.0, 1.80, 4.0])

    # ---- device side -------------------------------------------------------------------------------------------------
    def _on_device(self, mesh):
        return mesh if isinstance(mesh, _DeviceMesh) else _DeviceMesh(mesh, self.device)

    def _grid(self, pmin, pmax, shape, generator):
        lo = torch.as_tensor(pmin, dtype=torch.float32).to(self.device)
        hi = torch.as_tensor(pmax, dtype=torch.float32).to(self.device)
        u = torch.rand(tuple(shape) + (3,), device=self.device, dtype=torch.float32, generator=generator)
        return torch.minimum(lo + u * (hi - lo), hi)

    def _draw(self, smpl_v, smpl_f, obj_v, obj_f, sigma, n_surface, n_grid, generator):
        """(B, n_surface + n_grid, 3): surface samples of body and object as ONE mesh + sigma N(0,1), then grid points"""
        comb_v = torch.cat([smpl_v, obj_v], 1)
        comb_f = torch.cat([smpl_f.long(), obj_f.long() + smpl_v.shape[1]], 0)
        pts, _ = sample_surface(comb_v, comb_f, n_surface, generator)
        pts = pts + sigma * torch.randn(pts.shape, device=self.device, dtype=torch.float32, generator=generator)
        pmin, pmax = BoundarySampler.get_bounds()
        return torch.cat([pts, self._grid(pmin, pmax, (pts.shape[0], n_grid), generator)], 1)

    def train_batch(self, smpl_verts, smpl_faces, obj_verts, obj_faces, body_center, total_samplenum=20000,
                    sigmas=(0.08, 0.02, 0.003), ratios=(0.01, 0.49, 0.5), grid_ratio=0.01, pca_axis=None, generator=None):
        """The targets of one training step from meshes on the device, under CHORE.forward's keyword names:
        points (B,N,3), df_h, df_o (B,N), parts_gt (B,N) int64, pca_gt (B,3,3,N), body_center (B,3), obj_center (B,3,N)
        (object centre minus body centre, constant along N), N = total_samplenum.

        The N points are the mixture the reference reaches in two stages (a file of sample_num (1 + grid_ratio) points per
        sigma, of which data/train_data.py picks int(N * ratio) at random): per sigma int(N * ratio) points, the share
        grid_ratio / (1 + grid_ratio) of them -- 1 in 101 -- grid points; what the truncations leave of N goes to the last
        sigma.  smpl_verts (B,V,3), obj_verts (B,Vo,3), faces shared by the batch; pca_axis (B,3,3) or None = compute_pca of
        every object once per call (host, sklearn)."""
        dev = self.device
        g = self.generator if generator is None else generator
        sv = torch.as_tensor(smpl_verts, dtype=torch.float32, device=dev).detach()
        ov = torch.as_tensor(obj_verts, dtype=torch.float32, device=dev).detach()
        sf = torch.as_tensor(smpl_faces, device=dev).to(torch.int32)
        of = torch.as_tensor(obj_faces, device=dev).to(torch.int32)
        center = torch.as_tensor(body_center, dtype=torch.float32, device=dev)
        B, N = sv.shape[0], int(total_samplenum)
        counts = [int(N * r) for r in ratios]
        counts[-1] += N - sum(counts)
        groups = []
        for s, n in zip(sigmas, counts):
            n_grid = int(n * grid_ratio / (1.0 + grid_ratio))
            groups.append(self._draw(sv, sf, ov, of, s, n - n_grid, n_grid, g))
        points = torch.cat(groups, 1).contiguous()
        df_h, vid = mesh_distance(points, sv, sf, ("dist", "vert_idx"))
        df_o = mesh_distance(points, ov, of, "dist")
        parts = self._labels_on_device()[vid.long()]
        if pca_axis is None:
            ov_host = ov.double().cpu().numpy()
            pca_axis = np.stack([BoundarySampler.compute_pca(SimpleNamespace(v=v)) for v in ov_host])
        pca = torch.as_tensor(np.asarray(pca_axis, np.float32) if not torch.is_tensor(pca_axis) else pca_axis,
                              dtype=torch.float32, device=dev).reshape(B, 3, 3)
        obj_center = ov.mean(1) - center
        return {
            "points": points, "df_h": df_h, "df_o": df_o, "parts_gt": parts,
            "pca_gt": pca[:, :, :, None].expand(B, 3, 3, N).contiguous(),
            "body_center": center,
            "obj_center": obj_center[:, :, None].expand(B, 3, N).contiguous(),
        }
