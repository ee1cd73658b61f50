"""Fitting maths of CHORE on the GPU: SO(3) projection, object transform, loss terms.

Counterpart of /root/reference/recon/recon_fit_base.py (ReconFitterBase) for the methods that sit on the
optimisation hot path; file I/O and dataset glue of that class are out of scope; its mesh viewer (-d) is
replaced by headless point-cloud views (visualize_*, at the end of the class).
Method names, signatures and loss-dict keys are the reference's, so recon_fit_behave-style drivers read
the same.  Heavy steps run in libchore_hip.so: the field queries (chore_query_fwd/bwd_points), SMPL-H LBS
(chore_smpl_lbs_*) and the SO(3) projection (chore_so3_project_*); the remaining terms are a few
reductions over (B,N) tensors expressed with torch ops on the device.
"""
import json
import os
import threading
import pickle as pkl

import numpy as np
import torch
import torch.nn.functional as F

from .. import _lib
from ..lib_smpl.const import SMPL_PARTS_NUM, SMPL_POSE_PRAMS_NUM  # noqa: F401
from ..lib_smpl.wrapper_pytorch import SMPLPyTorchWrapperBatchSplitParams
from ..model.camera import KinectColorCamera
from . import fit_terms
from ..utils.paths import BEHAVE_PATH, RECON_PATH, SMPL_ASSETS_ROOT  # noqa: F401  (names the reference's scripts import from here, recon_fit_base.py:39-45)


# 14 body-part colours of the visualisations (recon/opt_utils.py:13-28)
MTURK_COLORS = np.array([44, 160, 44, 31, 119, 180, 255, 127, 14, 214, 39, 40, 148, 103, 189, 140, 86, 75, 227, 119, 194,
                         127, 127, 127, 189, 189, 34, 255, 152, 150, 23, 190, 207, 174, 199, 232, 255, 187, 120, 152, 223,
                         138]).reshape((-1, 3)) / 255.


def write_ply(path, verts, faces=None):
    """binary little-endian PLY (float32 vertices, int32 triangle lists)"""
    verts = np.asarray(verts, "<f4")
    with open(path, "wb") as f:
        hdr = ["ply", "format binary_little_endian 1.0", f"element vertex {len(verts)}", "property float x",
               "property float y", "property float z"]
        if faces is not None:
            hdr += [f"element face {len(faces)}", "property list uchar int vertex_indices"]
        f.write(("\n".join(hdr) + "\nend_header\n").encode("ascii"))
        f.write(verts.tobytes())
        if faces is not None:
            rec = np.zeros(len(faces), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
            rec["n"], rec["v"] = 3, np.asarray(faces)
            f.write(rec.tobytes())


# The CPU random stream the optimisation of the batch fitted by THIS host thread draws from (the SO(3) perturbations): None = the
# process-wide generator, like the reference; fit_recon with `batch_seed` gives every batch a generator of its own, so that
# batches fitted side by side (recon_fit_behave._fit_concurrent) draw what they draw in the serial loop.
_BATCH_RNG = threading.local()


def cpu_generator():
    return getattr(_BATCH_RNG, "gen", None)


class _SO3Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mat):
        B = mat.shape[0]
        dev = mat.device
        h = _lib.handle(dev.index or 0)
        m = mat.float().contiguous()
        R = torch.empty_like(m)
        aux = torch.empty(_lib.lib.chore_so3_aux_bytes(B), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.lib.chore_so3_project_fwd(h, m.data_ptr(), B, R.data_ptr(), aux.data_ptr(), stream), h,
                   "chore_so3_project_fwd")
        ctx.save_for_backward(aux)
        return R

    @staticmethod
    def backward(ctx, g):
        aux, = ctx.saved_tensors
        B = g.shape[0]
        dev = g.device
        h = _lib.handle(dev.index or 0)
        g = g.float().contiguous()
        dM = torch.empty_like(g)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.lib.chore_so3_project_bwd(h, aux.data_ptr(), g.data_ptr(), B, dM.data_ptr(), stream), h,
                   "chore_so3_project_bwd")
        return dM


class _ContactFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hum, obj, df_hum_o, df_obj_h, part_logits, label_h, thres):
        dev = hum.device
        if not hum.is_cuda:
            raise RuntimeError("chore_amd needs device tensors (no CPU path)")
        h = _lib.handle(dev.index or 0)
        B, Nh, _ = hum.shape
        No, P = obj.shape[1], part_logits.shape[1]
        hum_c, obj_c = hum.detach().float().contiguous(), obj.detach().float().contiguous()
        lab = label_h.to(device=dev, dtype=torch.int32).contiguous()
        ws = torch.empty(_lib.lib.chore_contact_workspace_bytes(B, Nh, No, P), dtype=torch.uint8, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        # keep the converted inputs in locals until the launch is enqueued: a temporary freed inside the argument
        # list hands its block to the next temporary and the two pointers alias
        dfh, dfo = df_hum_o.float().contiguous(), df_obj_h.float().contiguous()
        logits = part_logits.float().contiguous()
        _lib.check(_lib.lib.chore_contact_fwd(h, hum_c.data_ptr(), obj_c.data_ptr(), dfh.data_ptr(), dfo.data_ptr(),
                                              lab.data_ptr(), logits.data_ptr(), B, Nh, No, P, float(thres),
                                              loss.data_ptr(), ws.data_ptr(), stream), h, "chore_contact_fwd")
        ctx.save_for_backward(hum_c, obj_c, lab, ws)
        ctx.P = P
        return loss

    @staticmethod
    def backward(ctx, g):
        hum, obj, lab, ws = ctx.saved_tensors
        dev = hum.device
        h = _lib.handle(dev.index or 0)
        B, Nh, _ = hum.shape
        No = obj.shape[1]
        # a cloud that is a constant of the caller (the body in optimize_smpl_object) gets no gradient: NULL skips its kernels
        d_hum = torch.empty_like(hum) if ctx.needs_input_grad[0] else None
        d_obj = torch.empty_like(obj) if ctx.needs_input_grad[1] else None
        if d_hum is None and d_obj is None:
            return (None,) * 7
        g = g.float().contiguous()
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.lib.chore_contact_bwd(h, hum.data_ptr(), obj.data_ptr(), lab.data_ptr(), B, Nh, No, ctx.P,
                                              g.data_ptr(), ws.data_ptr(), None if d_hum is None else d_hum.data_ptr(),
                                              None if d_obj is None else d_obj.data_ptr(), stream),
                   h, "chore_contact_bwd")
        return d_hum, d_obj, None, None, None, None, None


class _CollisionFn(torch.autograd.Function):
    """per-batch interpenetration sums of a triangle mesh (chore_collision_fwd / _bwd, csrc/collision.hip)"""

    @staticmethod
    def forward(ctx, verts, faces):
        dev = verts.device
        if not verts.is_cuda:
            raise RuntimeError("chore_amd needs device tensors (no CPU path)")
        h = _lib.handle(dev.index or 0)
        B, V, _ = verts.shape
        F_ = faces.shape[0]
        vc = verts.detach().float().contiguous()
        ws = torch.empty(_lib.lib.chore_collision_workspace_bytes(B, V, F_), dtype=torch.uint8, device=dev)
        loss = torch.empty(B, dtype=torch.float32, device=dev)
        gverts = torch.empty(B, V, 3, dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.lib.chore_collision_fwd(h, vc.data_ptr(), faces.data_ptr(), B, V, F_, loss.data_ptr(),
                                                gverts.data_ptr(), None, ws.data_ptr(), stream), h, "chore_collision_fwd")
        ctx.save_for_backward(gverts)
        return loss

    @staticmethod
    def backward(ctx, g):
        (gverts,) = ctx.saved_tensors
        dev = gverts.device
        h = _lib.handle(dev.index or 0)
        B, V, _ = gverts.shape
        g = g.float().contiguous()
        dverts = torch.empty_like(gverts)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.lib.chore_collision_bwd(h, gverts.data_ptr(), g.data_ptr(), B, V, dverts.data_ptr(), stream), h,
                   "chore_collision_bwd")
        return dverts, None


class _Scan:
    """object template: .v (V,3) float64 centred vertices, .f (F,3) int64 faces (the two attributes of psbody's Mesh
    the reference uses)"""

    def __init__(self, v, f):
        self.v, self.f = np.asarray(v, np.float64), np.asarray(f, np.int64)


def sample_surface(verts, faces, count, rs):
    """`count` points uniformly on the triangle mesh (area-weighted triangle choice + uniform barycentric point) -- what
    trimesh.Trimesh.sample does (recon_fit_base.py:120-121), drawn from the numpy RandomState `rs`"""
    tri = verts[faces]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    idx = np.searchsorted(np.cumsum(area), rs.random_sample(count) * area.sum())
    idx = np.minimum(idx, len(faces) - 1)
    u, v = rs.random_sample(count), rs.random_sample(count)
    flip = u + v > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    t = tri[idx]
    return t[:, 0] + u[:, None] * (t[:, 1] - t[:, 0]) + v[:, None] * (t[:, 2] - t[:, 0])


class ReconFitterBase:
    def __init__(self, seq_folder=None, device="cuda:0", debug=False, obj_name=None, outpath=RECON_PATH, args=None,
                 assets=None):
        """the reference's argument list (recon_fit_base.py:48-52) + `assets`: where the files it reads come from
        (recon/assets.py; default: the folders of ./PATHS.yml like the reference).  Everything loaded here -- template
        PCA axes and surface samples, part labels, priors -- lands on the device once."""
        from .assets import FileAssets
        self.seq_folder, self.outpath = seq_folder, outpath
        self.assets = assets if assets is not None else FileAssets.from_paths_yml()
        info = self.assets.seq_info(seq_folder) if seq_folder is not None else None
        if info is None:
            if obj_name is None:
                raise AssertionError("must provide the name of the object to be reconstructed!")
            self.gender = "male"
        else:
            obj_name, self.gender = info
        self._init_common(device, debug)
        pca_init, obj_points = self.compute_pca_init(obj_name)
        self.pca_init = torch.tensor(pca_init, dtype=torch.float32).to(self.device)
        self.obj_points = torch.tensor(obj_points, dtype=torch.float32).to(self.device)
        self.part_labels = self.load_part_labels()
        crop = args.loadSize if args is not None else 1200
        self.camera = KinectColorCamera(crop)
        self.net_in_size = args.net_img_size[0] if args is not None else 512
        self.z_0 = 2.2 if args is None or "z_0" not in args else args.z_0
        self.scan_verts = torch.as_tensor(self.scan.v, dtype=torch.float32, device=self.device)
        self.scan_faces = torch.as_tensor(self.scan.f, dtype=torch.long, device=self.device)
        self.body_prior, self.hand_prior = self.assets.priors(self.device)

    def _init_common(self, device, debug):
        self.device = torch.device(device)
        self.debug = debug
        self.obj_scale = 1.0
        self.scan = None
        self.scan_verts = self.scan_faces = None
        self._comb_faces = None
        self._layers = {}
        self.part_names = {0: "head", 1: "left foot", 2: "left hand", 3: "left leg", 4: "left midarm",
                           5: "left upper arm", 6: "right foot", 7: "right hand", 8: "right leg", 9: "right midarm",
                           10: "right right upper arm", 11: "torso", 12: "upper left leg", 13: "upper right leg"}

    @classmethod
    def from_parts(cls, device="cuda:0", net_in_size=512, crop_size=1200, z_0=2.2, obj_scale=1.0, part_labels=None,
                   body_prior=None, hand_prior=None, debug=False, scan_verts=None, scan_faces=None, assets=None):
        """a fitter from values already in memory (tests, benchmarks): no sequence folder, no files"""
        self = cls.__new__(cls)
        self.seq_folder = self.outpath = None
        self.assets, self.gender = assets, "male"
        self._init_common(device, debug)
        if scan_verts is not None:
            self.scan = _Scan(np.asarray(torch.as_tensor(scan_verts).cpu()), np.asarray(torch.as_tensor(scan_faces).cpu()))
            self.scan_verts = torch.as_tensor(scan_verts, dtype=torch.float32, device=device)
            self.scan_faces = torch.as_tensor(scan_faces, dtype=torch.long, device=device)
        self.camera = KinectColorCamera(crop_size)
        self.net_in_size, self.z_0, self.obj_scale = net_in_size, z_0, obj_scale
        self.part_labels = part_labels          # (6890,) long: assets/smpl_parts_dense.pkl in the reference
        self.body_prior, self.hand_prior = body_prior, hand_prior
        return self

    # ---- what the reference loads from files ---------------------------------------------------------
    def compute_pca_init(self, obj_name, n_samples=3000, seed=0):
        """template -> centred mesh (self.scan), its PCA axes (3,3) and 3 000 surface samples  [recon_fit_base.py:108-122]
        PCA = sklearn's, like the reference (its sign convention fixes which of the +-axes the object starts from)"""
        from sklearn.decomposition import PCA
        v, f = self.assets.template(obj_name)
        v = np.asarray(v, np.float64)
        v = v - np.mean(v, 0)          # load_scan_centered
        v = v - np.mean(v, 0)          # and once more in compute_pca_init (:115)
        self.scan = _Scan(v, f)
        pca = PCA(n_components=3)
        pca.fit(v)
        return pca.components_, sample_surface(self.scan.v, self.scan.f, n_samples, np.random.RandomState(seed))

    def load_part_labels(self):
        return torch.tensor(np.asarray(self.assets.part_labels(), np.int32)).to(self.device)

    def load_part_labels_batch(self, batch_size):
        return self.load_part_labels().repeat(batch_size, 1).to(self.device).long()

    def load_mocap(self, file):
        return self.assets.load_mocap(file)

    def smpl_layer(self, gender):
        """one packed body model per gender, kept on the device"""
        if gender not in self._layers:
            from ..lib_smpl.smpl_layer import SMPL_Layer
            self._layers[gender] = SMPL_Layer.from_arrays(self.assets.smpl_model(gender), gender=gender).to(self.device)
        return self._layers[gender]

    def get_smpl_init(self, image_paths, trans):
        """SMPL-H initialised from the FrankMocap prediction next to every image  [recon_fit_base.py:124-140]"""
        from ..lib_smpl.smpl_generator import SMPLHGenerator
        poses, betas = [], []
        for x in image_paths:
            p, b = self.load_mocap(x.replace(".color.jpg", ".mocap.json"))
            poses.append(p)
            betas.append(b)
        return SMPLHGenerator.get_smplh(np.stack(poses, 0), np.stack(betas, 0), trans, self.gender, device=self.device,
                                        assets=self.assets, layer=self.smpl_layer(self.gender))

    def get_kpt_paths(self, image_paths):
        return [x.replace(".color.jpg", ".color.json") for x in image_paths]

    def load_kpts(self, json_paths, tol):
        """(B,25,3) 2-D body keypoints in the original image, confidences below `tol` zeroed  [:305-320]"""
        kpts = []
        for file in json_paths:
            J2d = np.array(self.assets.load_kpts(file), np.float64).reshape((-1, 3))
            J2d[:, 2][J2d[:, 2] < tol] = 0
            kpts.append(J2d)
        return torch.tensor(np.stack(kpts, 0), dtype=torch.float32).to(self.device)

    def get_body_kpts2d(self, traindata_paths, tol=0.3):
        return self.load_kpts(self.get_kpt_paths(traindata_paths), tol)

    def get_parts_colors(self, part):
        """(B,N) labels -> (B,N,3) colours, visualisation only  [:652-659]"""
        part = part.cpu().numpy() if torch.is_tensor(part) else np.asarray(part)
        return MTURK_COLORS[np.clip(part, 0, 13)]

    def prepare_query_dict(self, batch):
        return {"crop_center": batch.get("crop_center").to(self.device)}

    def prep_smplfit(self, data, generator, pc_generated):
        """everything optimize_smpl needs, from a loader batch and the generated point clouds  [recon_fit_base.py:398-440]"""
        batch_size = data["images"].shape[0]
        human_points = pc_generated["human"]["points"].clone().detach().to(self.device)
        obj_points = pc_generated["object"]["points"].clone().detach().to(self.device)
        human_parts = pc_generated["human"]["parts"].clone().detach().to(self.device)
        human_t = pc_generated["human"]["centers"][:, :3]
        human_t[:, 2] = self.z_0                                   # in place, like the reference: fixed SMPL depth
        smpl = self.get_smpl_init(data.get("path"), human_t)
        part_labels = self.load_part_labels_batch(batch_size)
        part_colors = self.get_parts_colors(pc_generated["human"]["parts"])
        body_kpts = self.get_body_kpts2d(data.get("path"))
        body_kpts = self.scale_body_kpts(body_kpts, data.get("resize_scale").to(self.device),
                                         data.get("crop_scale").to(self.device), data.get("old_crop_center").to(self.device))
        body_kpts = body_kpts.clone().float().to(self.device)
        query_dict = self.prepare_query_dict(data)
        betas_dict = {"images": data.get("images").to(self.device), "human_init": human_points, "human_parts": human_parts,
                      "part_labels": part_labels, "part_colors": part_colors, "body_kpts": body_kpts,
                      "query_dict": query_dict, "net": generator.model,
                      "pose_init": smpl.pose[:, 3:SMPL_POSE_PRAMS_NUM].clone().detach().to(self.device)}
        return (betas_dict, body_kpts, human_parts, human_points, human_t, obj_points, part_colors, part_labels, query_dict,
                smpl)

    def init_obj_fit_data(self, batch_size, human_t, pc_generated, scale):
        """object translation from the predicted centres (relative to the SMPL centre), rotation from the predicted PCA
        axes against the template's, scale from the SMPL height ratio  [recon_fit_base.py:720-747]"""
        obj_t = pc_generated["object"]["centers"][:, 3:].to(self.device) + human_t.to(self.device)
        obj_t = obj_t.clone().detach().to(self.device).requires_grad_(True)
        pca_axis = pc_generated["object"]["pca_axis"].to(self.device)
        pca_axis_init = torch.stack([self.pca_init for _ in range(batch_size)], 0)
        obj_R = self.init_object_orientation(pca_axis, pca_axis_init).detach().requires_grad_(True)
        obj_s = scale.clone().detach().to(self.device).requires_grad_(True)
        object_init = torch.stack([self.obj_points for _ in range(batch_size)], 0)
        return obj_R, obj_s, obj_t, object_init

    # ---- results on disk (recon_fit_base.py:233-275) ---------------------------------------------------
    def get_output_paths(self, image_paths, save_name, test_id):
        seq_names = [x.split(os.sep)[-3] for x in image_paths]
        frame_times = [x.split(os.sep)[-2] for x in image_paths]
        smpl_files, obj_files = [], []
        for seq, frame in zip(seq_names, frame_times):
            folder = os.path.join(self.outpath, seq, frame, save_name)
            os.makedirs(folder, exist_ok=True)
            smpl_files.append(os.path.join(folder, f"k{test_id}.smpl.ply"))
            obj_files.append(os.path.join(folder, f"k{test_id}.object.ply"))
        return smpl_files, obj_files

    def is_done(self, image_paths, save_name, test_id):
        smpl_files, obj_files = self.get_output_paths(image_paths, save_name, test_id)
        return all(os.path.isfile(sf) and os.path.isfile(of) for sf, of in zip(smpl_files, obj_files))

    def save_outputs(self, smpl, obj_R, obj_t, traindata_paths, save_name, test_id, obj_s=None, images=None, crop_centers=None):
        """fitted SMPL mesh + parameters and object mesh + parameters next to each other  [:258-275, opt_utils.py:73-101];
        images (B,5,H,W) / crop_centers (B,2): the batch's, read by REPORT_DEPTH_ORDER and EXPORT_TEXTURED_OBJ only"""
        smpl_files, obj_files = self.get_output_paths(traindata_paths, save_name, test_id)
        smpl.forget()
        with torch.no_grad():
            verts = smpl()[0].cpu().numpy()
            faces = None if smpl.faces is None else smpl.faces.cpu().numpy()
            B = len(obj_files)
            obj_verts = self.scan_verts.unsqueeze(0).repeat(B, 1, 1)
            obj_verts = self.transform_object(obj_verts, obj_R, obj_t, obj_s).cpu().numpy()
            rot = self.decopose_axis(obj_R, no_rand=True).cpu().numpy()
        for i, (sf, of) in enumerate(zip(smpl_files, obj_files)):
            write_ply(sf, verts[i], faces)
            pkl.dump({"pose": smpl.pose[i].detach().cpu().numpy(), "betas": smpl.betas[i].detach().cpu().numpy(),
                      "trans": smpl.trans[i].detach().cpu().numpy(), "score": 0.0}, open(sf.replace(".ply", ".pkl"), "wb"))
            write_ply(of, obj_verts[i], self.scan.f)
            pkl.dump({"rot": rot[i], "trans": obj_t[i].detach().cpu().numpy(), "scale": obj_s[i].detach().cpu().numpy()},
                     open(of.replace(".ply", ".pkl"), "wb"))
        if self.REPORT_PENETRATION:             # of the very meshes written above; draws no random numbers
            if smpl.faces is None:
                raise RuntimeError("REPORT_PENETRATION needs the body model's faces")
            dev = self.device
            rep = self._penetration_of(torch.as_tensor(verts, device=dev), smpl.faces, torch.as_tensor(obj_verts, device=dev))
            rep = {k: None if v is None else {n: t.cpu().tolist() for n, t in v.items()} for k, v in rep.items()}
            for i, sf in enumerate(smpl_files):
                frame = {k: None if v is None else {n: x[i] for n, x in v.items()} for k, v in rep.items()}
                with open(sf.replace(".smpl.ply", ".penetration.json"), "w") as f:
                    json.dump(frame, f, indent=1)
        if self.REPORT_DEPTH_ORDER:             # of the fitted body and pose against the batch's masks; draws no random numbers
            if smpl.faces is None or images is None or crop_centers is None or obj_s is None:
                raise RuntimeError("REPORT_DEPTH_ORDER needs the body model's faces, obj_s, and the batch's images and crop centres")
            dev = self.device
            images = torch.as_tensor(images).to(dev)
            counts = self.depth_order_report(torch.as_tensor(verts, device=dev), smpl.faces, self.decopose_axis(obj_R, no_rand=True),
                                             obj_t, obj_s, images[:, 3, :, :], images[:, 4, :, :],
                                             torch.as_tensor(crop_centers).to(dev)).cpu().tolist()
            for i, sf in enumerate(smpl_files):
                with open(sf.replace(".smpl.ply", ".depth_order.json"), "w") as f:
                    json.dump(self.depth_order_frame(counts[i]), f, indent=1)
        if self.REPORT_OCCLUSION:               # of the very meshes written above; draws no random numbers
            from .eval.occlusion import COUNT_KEYS, frame_report
            if smpl.faces is None:
                raise RuntimeError("REPORT_OCCLUSION needs the body model's faces")
            dev = self.device
            rep = self._occlusion_of(torch.as_tensor(verts, device=dev), smpl.faces, torch.as_tensor(obj_verts, device=dev))
            counts = [rep[k].cpu().tolist() for k in COUNT_KEYS]
            for i, sf in enumerate(smpl_files):
                with open(sf.replace(".smpl.ply", ".occlusion.json"), "w") as f:
                    json.dump(frame_report(*[c[i] for c in counts]), f, indent=1)
        if self.EXPORT_TEXTURED_OBJ:            # the very meshes written above, wearing the photo; draws no random numbers
            if faces is None or images is None or crop_centers is None:
                raise RuntimeError("EXPORT_TEXTURED_OBJ needs the body model's faces and the batch's images and crop centres")
            self._export_textured_obj(smpl_files, obj_files, verts, faces, obj_verts, images, crop_centers)

    # ---- the fitted meshes as textured OBJ files (render/obj_io.py) ----------------------------------------------
    # True: save_outputs (given the batch's images and crop centres) also writes k{test_id}.smpl.obj / .mtl / .png and
    # k{test_id}.object.obj / .mtl / .png next to the PLY files: the vertices of the PLYs with the texture cubes
    # utils/render_utils.render_photo_views draws (photo_mesh_textures), as a texture atlas any mesh viewer opens.  A texel the
    # network's camera does not see has SMPL_OBJ_COLOR_LIST's colour, without the side view's light.  The fit itself never
    # reads them: no fitted bit changes.
    EXPORT_TEXTURED_OBJ = False

    def _export_textured_obj(self, smpl_files, obj_files, verts, faces, obj_verts, images, crop_centers):
        from ..render import save_obj
        from ..utils.render_utils import SMPL_OBJ_COLOR_LIST, Mesh, mesh_tensors, photo_mesh_textures
        dev = self.device
        images, crop_centers = torch.as_tensor(images).to(dev), torch.as_tensor(crop_centers).to(dev)
        for i, (sf, of) in enumerate(zip(smpl_files, obj_files)):
            meshes = [Mesh(v=verts[i], f=faces), Mesh(v=obj_verts[i], f=self.scan.f)]
            with torch.no_grad():
                v, f, colour = mesh_tensors(meshes, SMPL_OBJ_COLOR_LIST, dev)
                textures = photo_mesh_textures(images[i], crop_centers[i], v, f, colour[:, :, 0, 0, 0, :],
                                               depth_bias=self.VIEW_POINT_BIAS, camera=self.camera)[0]
            save_obj(sf.replace(".ply", ".obj"), verts[i], faces, textures[:len(faces)])
            save_obj(of.replace(".ply", ".obj"), obj_verts[i], self.scan.f, textures[len(faces):])

    # ---- how much of the fitted object the fitted body hides (recon/eval/occlusion.py) --------------------------
    # The reference skips a frame whose object is less than 30 % visible (recon/evaluate.py:53-58) and reads that from mask
    # files of the dataset.  Here it comes from the fit's own meshes through the Kinect colour camera.
    # True: save_outputs also writes k{test_id}.occlusion.json (one frame's counts, fractions and object_evaluated) next to
    # the PLY files.  The fit itself never reads it: no fitted bit changes.
    REPORT_OCCLUSION = False

    def _occlusion_of(self, smpl_verts, smpl_faces, obj_verts):
        from .eval.occlusion import occlusion
        if self.scan_faces is None:
            raise RuntimeError("occlusion_report needs the object template mesh (scan_verts / scan_faces)")
        return occlusion(smpl_verts, smpl_faces, obj_verts, self.scan_faces)

    def occlusion_report(self, smpl_verts, smpl_faces, obj_R, obj_t, obj_s):
        """the arguments of penetration_report -> per-frame device tensors body_visible / body_full / object_visible /
        object_full (int64 pixels of the frame), body_fraction / object_fraction (float64, NaN where nothing is covered):
        recon/eval/occlusion.py.  No gradient."""
        if self.scan_verts is None:
            raise RuntimeError("occlusion_report needs the object template mesh (scan_verts / scan_faces)")
        with torch.no_grad():
            scan = self.scan_verts.unsqueeze(0).expand(obj_R.shape[0], -1, -1)
            verts = self.transform_obj_verts(scan, obj_R.detach(), obj_t.detach(), obj_s.detach())
        return self._occlusion_of(smpl_verts.detach(), smpl_faces, verts)

    # ---- how far the fitted meshes sit inside each other (recon/eval/penetration.py) ------------------------
    # Not in the reference.  An exact measure, independent of the interpenetration term, of what that term is there to reduce:
    # vertices of one mesh inside the other by winding number, depth by the exact distance to the other's surface.
    # True: save_outputs also writes k{test_id}.penetration.json (one frame's penetration_report) next to the PLY files.
    # The fit itself never reads it: no fitted bit changes.
    REPORT_PENETRATION = False

    # True: forward_step(..., "joint") adds loss_dict["pen"] = compute_penetration_loss after "collide" (when there is a
    # template mesh).  An exact, differentiable restatement of what the report prints, weighted by get_loss_weights()["pen"].
    # False (the default): nothing is computed, no key appears, no fitted bit changes.
    PENETRATION_TERM = False

    # True: optimize_smpl_object builds the silhouette term from the batch's masks with SilLossROI.from_masks (boxes, crops,
    # intrinsics and the edge distance transform on the device, no host round trip) and a kept slot refreshes its term in place
    # with set_masks.  The crops are then sampled in float64, not float32: pixels within round-off of the threshold can differ.
    # False (the default): the host constructor, as before; no fitted bit changes.
    SIL_DEVICE_SETUP = False
    SIL_REND_SIZE = 256         # the term's rend_size when this class builds it (the reference's default)

    # True: forward_step(..., "sil") adds loss_dict["edge"] = SilLossROI.edge_loss of the image the mask term rendered
    # (PHOSA's sum(edges(rendered) * edt_ref_edge), which pulls the rendered outline onto the mask's), weighted by
    # get_loss_weights()["edge"].  False (the default): nothing is computed, no key appears, no fitted bit changes.
    SIL_EDGE_TERM = False

    # True: optimize_smpl_object fills the silhouette term's occluder once per call (SilLossROI.set_occluder(body, faces): the
    # body's depth image over the ROI cameras; the body does not move there and gets no gradient), and forward_step adds
    # loss_dict["depth"] = SilLossROI.depth_loss -- PHOSA's ordinal depth term: where the person mask shows, the body is in
    # front of the object; where the object mask shows, the object is -- in the 'sil' phase after "edge" (on the placement and
    # rasterisation of the mask term) and in the 'joint' phase after "pen" (on its own), weighted by
    # get_loss_weights()["depth"].  It needs SilLossROI's device path: a silhouette term without set_occluder, or
    # CHORE_SIL_TORCH_PROJECT in the environment, is refused by optimize_smpl_object before any step.
    # False (the default): nothing is computed, no key appears, no fitted bit changes.
    ORDINAL_DEPTH_TERM = False

    # True: save_outputs (given the batch's images and crop centres) also writes k{test_id}.depth_order.json next to the PLY
    # files: per frame the four pixel counts of the fitted meshes (depth_order_report) and the two violated fractions.  The fit
    # itself never reads it: no fitted bit changes.
    REPORT_DEPTH_ORDER = False

    def depth_order_report(self, smpl_verts, smpl_faces, obj_R, obj_t, obj_s, person_masks, obj_masks, crop_centers):
        """body vertices (B,V,3) and faces, the object pose (obj_R: rotation matrices), the (B,H,W) network-input masks and
        (B,2) crop centres -> (B,4) int32 device tensor: pixels of the silhouette term's grid in case A (a person pixel where the
        object is in front of the body), in case B (an object pixel where the body is in front), person pixels where both meshes
        project, object pixels where both do (chore_ordinal_depth_fwd's counts).  No gradient."""
        from .obj_pose_roi import SilLossROI
        if self.scan is None:
            raise RuntimeError("depth_order_report needs the object template mesh (scan_verts / scan_faces)")
        with torch.no_grad():
            sil = SilLossROI.from_masks(person_masks, obj_masks, self.scan, crop_centers, rend_size=self.SIL_REND_SIZE,
                                        device=self.device, crop_size=self.camera.crop_size)
            sil.set_occluder(smpl_verts.detach(), smpl_faces)
            return sil.depth_order_counts(obj_R.detach().float(), obj_t.detach().float(), obj_s.detach().float().reshape(-1))

    @staticmethod
    def depth_order_frame(counts4):
        """one frame's counts -> the report's dict; a fraction is None where its denominator is 0"""
        a, b, pb, ob = (int(x) for x in counts4)
        return {"person_pixels_object_in_front": a, "object_pixels_body_in_front": b, "person_pixels_both": pb,
                "object_pixels_both": ob, "person_violated_fraction": a / pb if pb else None,
                "object_violated_fraction": b / ob if ob else None}

    def _template_closed(self):
        """is the template a closed mesh (is_closed)?  Checked on the host once per template -- before any step is recorded"""
        from .eval.penetration import is_closed
        if getattr(self, "_scan_closed", None) is None or self._scan_closed[0] is not self.scan_faces:
            self._scan_closed = (self.scan_faces, is_closed(self.scan_faces))          # host, once per template
        return self._scan_closed[1]

    def _penetration_of(self, smpl_verts, smpl_faces, obj_verts):
        from .eval.penetration import penetration
        if self.scan_faces is None:
            raise RuntimeError("penetration_report needs the object template mesh (scan_verts / scan_faces)")
        closed = self._template_closed()
        with torch.no_grad():
            out = {"object_in_body": penetration(smpl_verts, smpl_faces, obj_verts), "body_in_object": None}
            if closed:
                out["body_in_object"] = penetration(obj_verts, self.scan_faces, smpl_verts)
        return out

    def compute_penetration_loss(self, smpl_verts, smpl_faces, obj_R, obj_t, obj_s):
        """the arguments of compute_collision_loss -> the mean over the frames of penetration_loss(body, smpl_faces, template)
        [template vertices inside the body] + penetration_loss(template, scan_faces, body) [body vertices inside the template;
        only when the template is a closed mesh, _penetration_of's rule]: per direction frac * mean_depth of
        penetration_report, in metres.  Differentiable in the body and in obj_R / obj_t / obj_s (recon/eval/penetration.py)."""
        from .eval.penetration import penetration_loss
        if self.scan_verts is None or self.scan_faces is None:
            raise RuntimeError("compute_penetration_loss needs the object template mesh (scan_verts / scan_faces)")
        closed = self._template_closed()
        scan = self.scan_verts.unsqueeze(0).expand(obj_R.shape[0], -1, -1)
        verts = self.transform_obj_verts(scan, obj_R, obj_t, obj_s)
        loss = penetration_loss(smpl_verts, smpl_faces, verts)
        if closed:
            loss = loss + penetration_loss(verts, self.scan_faces, smpl_verts)
        return loss.mean()

    def penetration_report(self, smpl_verts, smpl_faces, obj_R, obj_t, obj_s):
        """the arguments of compute_collision_loss (obj_R: rotation matrices) -> {"object_in_body": vertices of the transformed
        template inside the body, "body_in_object": body vertices inside the template, or None when the template is not a
        closed mesh (is_closed)}; each a dict of per-frame device tensors count / frac / max_depth / mean_depth
        (recon/eval/penetration.py).  The body mesh is taken to be closed, as SMPL's is.  No gradient."""
        if self.scan_verts is None:
            raise RuntimeError("penetration_report needs the object template mesh (scan_verts / scan_faces)")
        with torch.no_grad():
            scan = self.scan_verts.unsqueeze(0).expand(obj_R.shape[0], -1, -1)
            verts = self.transform_obj_verts(scan, obj_R.detach(), obj_t.detach(), obj_s.detach())
        return self._penetration_of(smpl_verts.detach(), smpl_faces, verts)

    # ---- SO(3) ------------------------------------------------------------------------------------
    @staticmethod
    def project_so3(mat):
        """(B,3,3) -> closest rotation U diag(1,1,det(UV^T)) V^T   [recon_fit_base.py:168-188]"""
        if mat.shape[1:] != (3, 3):
            raise ValueError(f"invalid shape {tuple(mat.shape)}")
        if not mat.is_cuda:
            raise RuntimeError("chore_amd needs device tensors (no CPU path)")
        return _SO3Fn.apply(mat)

    @staticmethod
    def decopose_axis(rot, no_rand=False, noise=None):
        """[recon_fit_base.py:374-384] the 1e-4*U[0,1) perturbation is drawn with the CPU generator, like
        the reference (so seeded runs consume the same random stream); `noise` lets tests replay it"""
        if no_rand:
            return ReconFitterBase.project_so3(rot)
        if noise is None:
            noise = torch.rand(rot.shape[0], 3, 3, generator=cpu_generator())
        return ReconFitterBase.project_so3(rot + 1e-4 * noise.to(rot.device))

    @staticmethod
    def inverse(mat):
        tr = torch.bmm(mat.transpose(2, 1), mat)
        return torch.bmm(torch.inverse(tr), mat.transpose(2, 1))

    @staticmethod
    def init_object_orientation(tgt_axis, src_axis):
        return ReconFitterBase.decopose_axis(torch.bmm(ReconFitterBase.inverse(src_axis), tgt_axis))

    def transform_obj_verts(self, verts, obj_R, obj_t, obj_s):
        """rotate, translate, THEN scale (reference order, recon_fit_base.py:367-371)"""
        if fit_terms.obj_transform_supported(verts, obj_R, obj_t, obj_s):
            return fit_terms.obj_transform(verts, obj_R, obj_t, obj_s)     # one launch each way (csrc/fit_terms.hip)
        verts = torch.bmm(verts, obj_R) + obj_t.unsqueeze(1)
        return verts * obj_s.unsqueeze(1).unsqueeze(1)

    # ---- interpenetration (parity unpinned, see oracle/collision.py) --------------------
    def smpl_obj_collision(self, smpl_verts, smpl_faces, obj_verts, obj_faces):
        """mean over the batch of the penetration loss of the concatenated mesh   [recon_fit_base.py:610-624]"""
        comb_verts = torch.cat([smpl_verts, obj_verts], 1)
        key = (smpl_faces.data_ptr(), obj_faces.data_ptr(), smpl_verts.shape[1])
        if self._comb_faces is None or self._comb_faces[0] != key:
            comb = torch.cat([smpl_faces.to(self.device).long(), obj_faces.to(self.device).long() + smpl_verts.shape[1]], 0)
            self._comb_faces = (key, comb.to(torch.int32).contiguous())
        return torch.mean(_CollisionFn.apply(comb_verts, self._comb_faces[1]))

    def compute_collision_loss(self, smpl_verts, smpl_faces, obj_R, obj_t, obj_s):
        """collision loss between the SMPL and the object template mesh   [recon_fit_base.py:626-639]"""
        if self.scan_verts is None or self.scan_faces is None:
            raise RuntimeError("compute_collision_loss needs the object template mesh (scan_verts / scan_faces)")
        scan = self.scan_verts.unsqueeze(0).expand(obj_R.shape[0], -1, -1)
        verts = self.transform_obj_verts(scan, obj_R, obj_t, obj_s)
        return self.smpl_obj_collision(smpl_verts, smpl_faces, verts, self.scan_faces)

    def transform_object(self, object_init, rot, obj_t, obj_s):
        return self.transform_obj_verts(object_init, self.decopose_axis(rot), obj_t, obj_s)

    # ---- loss terms --------------------------------------------------------------------------------
    @staticmethod
    def sum_dict(loss_dict, weight_dict, it):
        """[recon_fit_behave.py:339-358] sum_k w_k(L_k, it) with w_k = c_k * L / (1 + it).  Inside the steppers `it` stands for
        a device scalar (graph_step._OnePlusDecay) and the terms are device scalars: one launch computes the sum and one its
        backward (csrc/fit_step.hip) instead of two tensor ops per term, a stack and a reduction, each way."""
        from .graph_step import _OnePlusDecay, weighted_sum
        vals = list(loss_dict.values())
        if isinstance(it, _OnePlusDecay) and vals and all(torch.is_tensor(v) and v.is_cuda and v.dim() == 0 and
                                                          v.dtype == torch.float32 for v in vals) and len(vals) <= 16:
            return weighted_sum(vals, [float(weight_dict[k](1.0, 0)) for k in loss_dict], it.denom)
        return torch.stack([weight_dict[k](v, it) for k, v in loss_dict.items()]).sum()

    def compute_obj_loss(self, data_dict, loss_dict, model, obj_s, object, preds=None, scale_term=True):
        """`preds`: the field at `object` when the caller has queried these very points already in this step (the
        reference queries them twice per step, recon_fit_behave.py:171,183 -> recon_fit_base.py:505-506, with the same
        result): one query forward and one backward instead of two"""
        if preds is None:
            model.query(object, **data_dict["query_dict"])
            preds = model.get_preds()
        if fit_terms.point_terms_supported(preds[0]):
            loss_dict["object"] = fit_terms.point_terms(preds[0], 1, 0.8)[0]
        else:
            loss_dict["object"] = torch.clamp(preds[0][:, 1:2, :], max=0.8).mean()
        if scale_term:
            loss_dict["scale"] = torch.mean((obj_s - self.obj_scale) ** 2)
        return preds

    def compute_prior_loss(self, loss_dict, smpl, nobeta=False):
        if not nobeta:
            loss_dict["beta"] = torch.mean(smpl.betas ** 2)
        loss_dict["pose"] = torch.mean(self.body_prior(smpl.pose[:, :72]))
        loss_dict["hand"] = torch.mean(self.hand_prior(smpl.pose))

    def compute_df_h_loss(self, data_dict, loss_dict, model, smpl_verts):
        model.query(smpl_verts, **data_dict["query_dict"])
        df_pred, _, parts_pred, centers_pred = model.get_preds()
        if fit_terms.point_terms_supported(df_pred):
            loss_dict["df_h"] = fit_terms.point_terms(df_pred, 0, 0.1)[0]
        else:
            loss_dict["df_h"] = torch.clamp(df_pred[:, 0:1, :], max=0.1).mean()
        return df_pred, parts_pred, centers_pred

    def compute_smpl_center_pred(self, data_dict, model, smpl):
        with torch.no_grad():
            verts = smpl()[0]
            model.query(verts, **data_dict["query_dict"])
            return torch.mean(model.get_preds()[3][:, :3], -1)

    def smplz_loss(self, J, loss_dict):
        loss_dict["smplz"] = torch.mean((J[:, 8, 2] - self.z_0) ** 2)

    def project_points(self, joints3d, crop_center=None):
        """3-D keypoints -> pixels of the network input image  [recon_fit_base.py:661-670]"""
        px, py = self.camera.project_screen(joints3d, crop_center)
        return torch.cat([px, py], -1) * self.net_in_size / self.camera.crop_size

    def projection_loss(self, joints3d, joints2d, crop_center):
        proj = self.project_points(joints3d, crop_center)
        loss = F.mse_loss(proj[:, :, :2], joints2d[:, :, :2], reduction="none")
        return torch.mean(torch.sum(loss, dim=-1) * joints2d[:, :, 2])

    def compute_kpts_loss(self, data_dict, loss_dict, smpl):
        J, _, _ = smpl.get_landmarks()
        loss_dict["j2d"] = self.projection_loss(J, data_dict["body_kpts"], data_dict["query_dict"]["crop_center"])

    def scale_body_kpts(self, kpts, resize_scale, crop_scale, crop_center):
        pxy = kpts[:, :, :2] * resize_scale.unsqueeze(1).unsqueeze(1)
        crop_org = crop_scale * self.camera.crop_size
        pxy = pxy - crop_center.unsqueeze(1) + crop_org.unsqueeze(1).unsqueeze(1) / 2
        pxy = pxy * self.net_in_size / crop_org.unsqueeze(1).unsqueeze(1)
        return torch.cat([pxy, kpts[:, :, 2:3]], -1)

    def compute_contact_loss(self, df_hum_o, df_obj_h, object, smpl_verts, loss_dict, part_o=None):
        """[recon_fit_base.py:553-608 + pytorch3d chamfer_distance :605-607] pair human / object contact points by
        part label and take the bidirectional squared nearest-neighbour distance -- one fixed-shape device
        computation (chore_contact_fwd/bwd) instead of per-frame, per-part Python loops over ragged clouds, so the
        step has no host synchronisation.  The term is always present; it is 0 where the reference omits it."""
        loss_dict["contact"] = _ContactFn.apply(smpl_verts, object, df_hum_o.detach(), df_obj_h.detach(),
                                                part_o.detach(), self.part_labels, 0.08)

    def split_smpl(self, smpl):
        return SMPLPyTorchWrapperBatchSplitParams.from_smpl(smpl)

    @staticmethod
    def copy_smpl_params(split_smpl, smpl):
        smpl.pose.data[:, :3] = split_smpl.global_pose.data
        smpl.pose.data[:, 3:66] = split_smpl.body_pose.data
        smpl.pose.data[:, 66:] = split_smpl.hand_pose.data
        smpl.betas.data[:, :2] = split_smpl.top_betas.data
        # the reference copies no other_betas here (:682-690) and does not need to: the split parameters are views of
        # smpl's storage (wrapper_pytorch.from_smpl), the optimised betas 2..9 are in smpl.betas already.  For a split
        # that owns its storage the line below keeps that outcome; for views it copies a tensor onto itself.
        smpl.betas.data[:, 2:] = split_smpl.other_betas.data
        smpl.trans.data = split_smpl.trans.data
        smpl.forget()   # writes through .data are invisible to the version counters the LBS memo is keyed on
        return smpl

    @staticmethod
    def get_smpl_height(smpl):
        with torch.no_grad():
            v = smpl()[0]
            return v[:, :, 1].max(1)[0] - v[:, :, 1].min(1)[0]

    # ---- looking at a fit (recon_fit_base.py:442-511, 704-718, 749-845) ---------------------------------
    # The reference opens a psbody MeshViewer and cv2 windows at every step; everything it shows is a point cloud.  Here the
    # same clouds are drawn headless by the point rasteriser (chore_splat_fwd through utils/render_utils.render_cloud_views)
    # and RETURNED as uint8 images of frame `_view_index` (0, like the reference's idx) of the batch.  Drawing draws no
    # random numbers and leaves the network's query state as it found it.
    VIEW_GREEN, VIEW_RED, VIEW_YELLOW, VIEW_BLUE = (0., 1., 0.), (1., 0., 0.), (1., 1., 0.), (0., 0., 1.)
    VIEW_CYAN, VIEW_MAGENTA = (0., 1., 1.), (1., 0., 1.)
    VIEW_VERT_R, VIEW_POINT_R = 0.005, 0.008      # world radii of SMPL vertices and of generated points, metres
    # visualize_fit_scene: opacity of the fitted meshes and of the ground-truth meshes, and how far (metres) a point may lie
    # behind a surface and still be drawn in front of it -- the generated points lie ON the surfaces they were fitted to
    VIEW_MESH_OPACITY, VIEW_GT_OPACITY, VIEW_POINT_BIAS = 0.6, 0.35, 0.02
    VIEW_CENTRE_R = 0.06                          # the centre markers of visualize_fit_scene: sphere meshes, metres
    # visualize_fit_scene: how many meshes a sample shows through each other (Renderer.render_scene's face_layers, one layer per
    # mesh).  1 = a translucent mesh hides every mesh behind it; set it to 4, say, to see the object through the body
    VIEW_FACE_LAYERS = 1
    # with -d, also write k{tid}.debug_photo.png per frame (visualize_photo_fit): the fitted meshes wearing the input photo
    VIEW_PHOTO_TEXTURES = False
    _view_index = 0
    debug_dest = None                             # (save_name, test_id) of the debug files; fit_recon sets it from its args

    def _cloud_views(self, data_dict, smpl, clouds, colors, radii):
        from ..utils.render_utils import CLOUD_VIEW_SIZE, render_cloud_views
        idx = self._view_index
        crop_center = data_dict["query_dict"]["crop_center"]
        with torch.no_grad():
            J, _, _ = smpl.get_landmarks()
            pxy = self.project_points(J, crop_center)[idx, :, :2] * (CLOUD_VIEW_SIZE / float(self.net_in_size))
        markers = [(pxy, self.VIEW_YELLOW, 3.0)]              # projected body-25 joints
        if "body_kpts" in data_dict:                          # detected keypoints
            markers.append((data_dict["body_kpts"][idx][:, :2] * (CLOUD_VIEW_SIZE / float(self.net_in_size)), self.VIEW_RED, 2.0))
        return render_cloud_views(data_dict["images"][idx], crop_center[idx], clouds, colors, radii, markers, camera=self.camera)

    def _human_clouds(self, data_dict, smpl_verts):
        idx = self._view_index
        parts = data_dict["part_colors"][idx] if "part_colors" in data_dict else \
            self.get_parts_colors(data_dict["human_parts"])[idx]
        return ([smpl_verts[idx].detach(), data_dict["human_init"][idx].detach()], [self.VIEW_GREEN, np.asarray(parts)],
                [self.VIEW_VERT_R, self.VIEW_POINT_R])

    def visualize_smpl_fit(self, data_dict, smpl, smpl_verts):
        """[:749-796] SMPL vertices (green), the generator's human points (part colours), contact vertices (blue, from
        `contact_mask`), the predicted SMPL centre as a 5 cm marker, the keypoints -> (512, 1152, 3) uint8"""
        idx = self._view_index
        clouds, colors, radii = self._human_clouds(data_dict, smpl_verts)
        if "contact_mask" in data_dict and bool(data_dict["contact_mask"][idx].any()):
            # first in the list: a contact vertex coincides with its SMPL vertex, and equal depths go to the smaller index
            clouds.insert(0, smpl_verts[idx, data_dict["contact_mask"][idx]].detach())
            colors.insert(0, self.VIEW_BLUE)
            radii.insert(0, self.VIEW_VERT_R)
        if "smpl_center_pred" in data_dict:
            clouds.append(data_dict["smpl_center_pred"][idx].detach().reshape(1, 3))
            colors.append(self.VIEW_YELLOW)
            radii.append(0.05)
        return self._cloud_views(data_dict, smpl, clouds, colors, radii)

    def visualize_fitting(self, data_dict, object, smpl, smpl_verts):
        """[:442-511] object points (red), their initial placement (yellow), SMPL vertices (green), the generator's human
        points (part colours), contact vertices and points (blue, from `contact_mask_h` / `contact_mask_o`), the centres
        `obj_center_pred` (cyan), `smpl_center_pred` (yellow) and `smpl_center_act` (magenta) as 6 cm markers, the
        keypoints -> (512, 1152, 3) uint8"""
        idx = self._view_index
        clouds, colors, radii = [], [], []
        for key, src in (("contact_mask_h", smpl_verts), ("contact_mask_o", object)):
            if key in data_dict and bool(data_dict[key][idx].any()):
                clouds.append(src[idx, data_dict[key][idx]].detach())
                colors.append(self.VIEW_BLUE)
                radii.append(self.VIEW_POINT_R)
        clouds += [object[idx].detach(), data_dict["obj_init"][idx].detach()]
        colors += [self.VIEW_RED, self.VIEW_YELLOW]
        radii += [self.VIEW_POINT_R, self.VIEW_POINT_R]
        hc, hcol, hr = self._human_clouds(data_dict, smpl_verts)
        clouds, colors, radii = clouds + hc, colors + hcol, radii + hr
        for key, colour in (("obj_center_pred", self.VIEW_CYAN), ("smpl_center_pred", self.VIEW_YELLOW),
                            ("smpl_center_act", self.VIEW_MAGENTA)):
            if key in data_dict:
                clouds.append(data_dict[key][idx].detach().reshape(1, 3))
                colors.append(colour)
                radii.append(0.06)
        return self._cloud_views(data_dict, smpl, clouds, colors, radii)

    def visualize_fit_scene(self, data_dict, object_verts, smpl, smpl_verts):
        """[:442-511, 749-795 in one view] the fitted meshes WITH the clouds they were fitted to, occluding each other per
        sample (chore_scene_fwd through utils/render_utils.render_scene_views): the fitted SMPL mesh and the object template
        under the fitted pose (`object_verts` (B,V,3) with self.scan_faces) in SMPL_OBJ_COLOR_LIST's colours, translucent;
        the generator's human points (part colours) and object points (red); contact vertices (blue, from `contact_mask_h`);
        the centres `obj_center_pred` (cyan), `smpl_center_pred` (yellow), `smpl_center_act` (magenta) as opaque 6 cm sphere
        meshes; `hum_gt` / `obj_gt` (objects with verts_list() / faces_list(), as the reference reads them) white and more
        translucent; the keypoints -> (512, 1152, 3) uint8.
        With VIEW_FACE_LAYERS = 1 (the default) a translucent face never shows another face, so a centre sphere inside a fitted
        mesh -- where the centres of a good fit lie -- is hidden by it.  Each centre is therefore ALSO a disc of the same radius at
        the centre's depth: a point, which the translucent mesh in front of it does show (blended), and which its own sphere
        covers wherever the sphere is visible.
        With VIEW_FACE_LAYERS = K > 1 (set it on the fitter or its class before fitting with -d) every sample composites its K
        nearest meshes front to back, each mesh one layer (chore_scene_layers_fwd with the mesh index as face group): the object,
        the ground-truth meshes and the centre spheres show through the body, and the duplicate discs are left out."""
        from ..utils.render_utils import (CLOUD_VIEW_SIZE, SMPL_OBJ_COLOR_LIST, Mesh, icosphere_mesh, render_scene_views)
        idx = self._view_index
        host = lambda x: np.asarray(x.detach().cpu()) if torch.is_tensor(x) else np.asarray(x)     # noqa: E731
        meshes, mesh_colors, opacity = [], [], []
        if smpl.faces is not None:
            meshes.append(Mesh(v=host(smpl_verts[idx]), f=host(smpl.faces)))
            mesh_colors.append(SMPL_OBJ_COLOR_LIST[0])
            opacity.append(self.VIEW_MESH_OPACITY)
        if object_verts is not None and self.scan_faces is not None:
            meshes.append(Mesh(v=host(object_verts[idx]), f=host(self.scan_faces)))
            mesh_colors.append(SMPL_OBJ_COLOR_LIST[1])
            opacity.append(self.VIEW_MESH_OPACITY)
        for key in ("hum_gt", "obj_gt"):
            if data_dict.get(key) is not None:
                meshes.append(Mesh(v=host(data_dict[key].verts_list()[idx]), f=host(data_dict[key].faces_list()[idx])))
                mesh_colors.append((1., 1., 1.))
                opacity.append(self.VIEW_GT_OPACITY)
        for key, colour in (("obj_center_pred", self.VIEW_CYAN), ("smpl_center_pred", self.VIEW_YELLOW),
                            ("smpl_center_act", self.VIEW_MAGENTA)):
            if key in data_dict:
                meshes.append(icosphere_mesh(host(data_dict[key][idx]).reshape(3), self.VIEW_CENTRE_R))
                mesh_colors.append(colour)
                opacity.append(1.0)
        clouds, colors, radii = [], [], []
        for key, colour in (("obj_center_pred", self.VIEW_CYAN), ("smpl_center_pred", self.VIEW_YELLOW),
                            ("smpl_center_act", self.VIEW_MAGENTA)):
            if key in data_dict and self.VIEW_FACE_LAYERS <= 1:
                clouds.append(data_dict[key][idx].detach().reshape(1, 3))
                colors.append(colour)
                radii.append(self.VIEW_CENTRE_R)
        if "contact_mask_h" in data_dict and bool(data_dict["contact_mask_h"][idx].any()):
            clouds.append(smpl_verts[idx, data_dict["contact_mask_h"][idx]].detach())
            colors.append(self.VIEW_BLUE)
            radii.append(self.VIEW_POINT_R)
        parts = data_dict["part_colors"][idx] if "part_colors" in data_dict else \
            self.get_parts_colors(data_dict["human_parts"])[idx]
        clouds += [data_dict["human_init"][idx].detach(), data_dict["obj_init"][idx].detach()]
        colors += [np.asarray(parts), self.VIEW_RED]
        radii += [self.VIEW_POINT_R, self.VIEW_POINT_R]
        crop_center = data_dict["query_dict"]["crop_center"]
        with torch.no_grad():
            J, _, _ = smpl.get_landmarks()
            pxy = self.project_points(J, crop_center)[idx, :, :2] * (CLOUD_VIEW_SIZE / float(self.net_in_size))
        markers = [(pxy, self.VIEW_YELLOW, 3.0)]              # projected body-25 joints
        if "body_kpts" in data_dict:                          # detected keypoints
            markers.append((data_dict["body_kpts"][idx][:, :2] * (CLOUD_VIEW_SIZE / float(self.net_in_size)), self.VIEW_RED, 2.0))
        return render_scene_views(data_dict["images"][idx], crop_center[idx], meshes, mesh_colors, opacity, clouds, colors, radii,
                                  markers, point_depth_bias=self.VIEW_POINT_BIAS, camera=self.camera,
                                  face_layers=self.VIEW_FACE_LAYERS)

    def visualize_photo_fit(self, data_dict, object_verts, smpl_verts, smpl_faces=None):
        """the fitted SMPL mesh (`smpl_verts` (B,V,3) with `smpl_faces` (F,3); left out without faces) and the object template under
        the fitted pose (`object_verts` (B,V,3) with self.scan_faces, or None) coloured from the input photo wherever the
        network's camera sees them, next to that photo
        (utils/render_utils.render_photo_views): a body slid along the viewing ray or a misplaced object wears the wrong patch of
        image.  Hidden texels keep SMPL_OBJ_COLOR_LIST's colours; VIEW_POINT_BIAS (metres, not tuned) is how far behind the
        nearest surface a texel may lie and still count as seen.  -> (512, 1152, 3) uint8"""
        from ..utils.render_utils import SMPL_OBJ_COLOR_LIST, Mesh, render_photo_views
        idx = self._view_index
        host = lambda x: np.asarray(x.detach().cpu()) if torch.is_tensor(x) else np.asarray(x)     # noqa: E731
        meshes, mesh_colors = [], []
        if smpl_faces is not None:
            meshes.append(Mesh(v=host(smpl_verts[idx]), f=host(smpl_faces)))
            mesh_colors.append(SMPL_OBJ_COLOR_LIST[0])
        if object_verts is not None and self.scan_faces is not None:
            meshes.append(Mesh(v=host(object_verts[idx]), f=host(self.scan_faces)))
            mesh_colors.append(SMPL_OBJ_COLOR_LIST[1])
        return render_photo_views(data_dict["images"][idx], data_dict["query_dict"]["crop_center"][idx], meshes, mesh_colors,
                                  depth_bias=self.VIEW_POINT_BIAS, camera=self.camera)

    def _contact_view_data(self, data_dict, model, obj_center_pred, object, smpl, smpl_verts):
        """what visualize_contact_fitting adds to data_dict for the whole batch: the contact masks (two field queries) and the
        three centres; the network's query state is restored"""
        kept = (model.preds, model.points, model.intermediate_preds_list)
        try:
            with torch.no_grad():
                model.query(smpl_verts, **data_dict["query_dict"])
                data_dict["contact_mask_h"] = model.get_preds()[0][:, 1, :] < 0.08
                model.query(object, **data_dict["query_dict"])
                data_dict["contact_mask_o"] = model.get_preds()[0][:, 0, :] < 0.08
                J, _, _ = smpl.get_landmarks()
                data_dict["obj_center_pred"] = obj_center_pred
                data_dict["smpl_center_pred"] = data_dict["smpl_center"]
                data_dict["smpl_center_act"] = J[:, 8]
        finally:
            model.preds, model.points, model.intermediate_preds_list = kept

    def visualize_contact_fitting(self, data_dict, edges, image, model, obj_center_pred, object, smpl, smpl_verts):
        """[:798-845] the contact masks from two field queries (at the SMPL vertices and at the object points, df < 0.08), the
        three centres, then visualize_fitting; with `image` / `edges` (the silhouette phase's rendering and edge map, with
        data_dict['image_ref'] / ['edt_ref']) the mask and edge panels are appended below.  Runs under no_grad and leaves
        model.preds / points / intermediate_preds_list as it found them.  -> (512 [+ h], 1152, 3) uint8"""
        idx = self._view_index
        self._contact_view_data(data_dict, model, obj_center_pred, object, smpl, smpl_verts)
        view = self.visualize_fitting(data_dict, object, smpl, smpl_verts)
        if image is None or edges is None:
            return view
        u8 = lambda x: (x[idx].detach().float().cpu().numpy() * 255).astype(np.uint8)     # noqa: E731
        img, img_ref, edt, edt_ref = u8(image), u8(data_dict["image_ref"]), u8(edges), u8(data_dict["edt_ref"])
        h, w = img.shape[:2]
        panels = np.zeros((h, max(2 * w, view.shape[1]), 3), np.uint8)
        panels[:, :w, 0], panels[:, :w, 2] = img_ref, img               # red: the reference mask, blue: the rendering
        panels[:, w:2 * w, 0], panels[:, w:2 * w, 2] = edt_ref, edt
        if panels.shape[1] > view.shape[1]:
            view = np.concatenate([view, np.zeros((view.shape[0], panels.shape[1] - view.shape[1], 3), np.uint8)], 1)
        return np.concatenate([view, panels], 0)

    def save_neural_recon(self, train_paths, recon_batch, save_name, tid):
        """[:704-718] the dense point clouds of a batch, one k{tid}_densepc.npz per frame: a dict per target ('human',
        'object') holding every entry of that target for the frame"""
        files = []
        for i, x in enumerate(train_paths):
            seq, frame = str(x).split(os.sep)[-3], str(x).split(os.sep)[-2]
            folder = os.path.join(self.outpath, seq, frame, save_name)
            os.makedirs(folder, exist_ok=True)
            out_dict = {}
            for tar in recon_batch:
                out_dict[tar] = {t: (v[i].detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v[i]))
                                 for t, v in recon_batch[tar].items()}
            files.append(os.path.join(folder, f"k{tid}_densepc.npz"))
            np.savez(files[-1], **out_dict)
        return files

    # the debug files of a batch, written BETWEEN the phases of the optimisation (never inside a recorded step)
    def _debug_files(self, image_paths, what):
        save_name, tid = self.debug_dest
        return [f.replace(".smpl.ply", f".debug_{what}.png") for f in self.get_output_paths(image_paths, save_name, tid)[0]]

    def _debug_on(self):
        return bool(self.debug) and self.outpath is not None and self.debug_dest is not None

    def debug_after_smpl(self, prep, data_dict, smpl):
        """after optimize_smpl: k{tid}.debug_smpl.png per frame and the dense clouds (save_neural_recon)"""
        if not self._debug_on():
            return
        from ..utils.render_utils import write_png
        paths = prep["data"]["path"]
        self.save_neural_recon(paths, prep["pc"], *self.debug_dest)
        model = prep["model"]
        kept = (model.preds, model.points, model.intermediate_preds_list)
        try:
            with torch.no_grad():
                smpl.forget()
                verts = smpl()[0]
                dd = dict(data_dict)
                dd["smpl_center_pred"] = self.compute_smpl_center_pred(data_dict, model, smpl)
                for i, f in enumerate(self._debug_files(paths, "smpl")):
                    self._view_index = i
                    write_png(f, self.visualize_smpl_fit(dd, smpl, verts))
        finally:
            self._view_index = 0
            model.preds, model.points, model.intermediate_preds_list = kept
            smpl.forget()

    def debug_after_object(self, prep, data_dict, smpl, obj_R, obj_t, obj_s):
        """after optimize_smpl_object: k{tid}.debug_object.png and k{tid}.debug_fit.png (visualize_fit_scene) per frame, and with
        VIEW_PHOTO_TEXTURES k{tid}.debug_photo.png (visualize_photo_fit)"""
        if not self._debug_on():
            return
        from ..utils.render_utils import write_png
        paths, model = prep["data"]["path"], prep["model"]
        kept = (model.preds, model.points, model.intermediate_preds_list)
        try:
            with torch.no_grad():
                smpl.forget()
                verts = smpl()[0]
                dd = dict(data_dict)
                if "smpl_center" not in dd:
                    dd["smpl_center"] = self.compute_smpl_center_pred(data_dict, model, smpl)
                object = self.transform_obj_verts(data_dict["objects"].detach(), self.decopose_axis(obj_R.detach(), no_rand=True),
                                                  obj_t.detach(), obj_s.detach())
                model.query(object, **data_dict["query_dict"])
                obj_center_pred = dd["smpl_center"] + torch.mean(model.get_preds()[3][:, 3:, :], -1)
                # what visualize_contact_fitting(dd, None, None, ...) draws, with the batch's queries made once for all frames
                self._contact_view_data(dd, model, obj_center_pred, object, smpl, verts)
                for i, f in enumerate(self._debug_files(paths, "object")):
                    self._view_index = i
                    write_png(f, self.visualize_fitting(dd, object, smpl, verts))
                scan = None
                if self.scan_verts is not None and self.scan_faces is not None:
                    scan = self.transform_obj_verts(self.scan_verts.unsqueeze(0).expand(obj_R.shape[0], -1, -1).contiguous(),
                                                    self.decopose_axis(obj_R.detach(), no_rand=True), obj_t.detach(), obj_s.detach())
                for i, f in enumerate(self._debug_files(paths, "fit")):
                    self._view_index = i
                    write_png(f, self.visualize_fit_scene(dd, scan, smpl, verts))
                if self.VIEW_PHOTO_TEXTURES:
                    for i, f in enumerate(self._debug_files(paths, "photo")):
                        self._view_index = i
                        write_png(f, self.visualize_photo_fit(dd, scan, verts, smpl.faces))
        finally:
            self._view_index = 0
            model.preds, model.points, model.intermediate_preds_list = kept
            smpl.forget()
