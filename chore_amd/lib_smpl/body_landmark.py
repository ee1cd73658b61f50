"""Body, face and hand landmarks of an SMPL mesh from the three sparse regressors under the SMPL assets folder.

Counterpart of the reference's lib_smpl/body_landmark.py, whose module imports psbody at the top: same class and method
names, host numpy / scipy.sparse only.  A mesh is any object with `.v` or `.vertices` (6 890 x 3)."""
import os
import pickle as pkl

import numpy as np


def load_regressors(assets_root, batch_size=None):
    """the (25, V), (70, V) and (42, V) scipy.sparse regressors of body25_regressor.pkl, face_regressor.pkl and
    hand_regressor.pkl (stored transposed).  With a batch_size: each as a stack of `batch_size` torch sparse tensors."""
    regs = []
    for name in ("body25", "face", "hand"):
        with open(os.path.join(assets_root, name + "_regressor.pkl"), "rb") as f:
            regs.append(pkl.load(f, encoding="latin1").T)
    if batch_size is None:
        return tuple(regs)
    import torch
    out = []
    for r in regs:
        coo = r.tocoo()
        t = torch.sparse_coo_tensor(np.stack([coo.row, coo.col]), coo.data, coo.shape)
        out.append(torch.stack([t] * batch_size))
    return tuple(out)


def _verts(mesh):
    return np.asarray(mesh.v if hasattr(mesh, "v") else mesh.vertices)


class BodyLandmarks:
    "landmarks of SMPL meshes: 25 body keypoints, 70 face and 42 hand landmarks; the body centre is keypoint 8"

    def __init__(self, assets_root):
        self.body25_reg, self.face_reg, self.hand_reg = load_regressors(assets_root)
        self.parts_inds = self.load_parts_ind(p=os.path.join(assets_root, "smpl_parts_dense.pkl"))

    def get_landmarks(self, smpl_mesh):
        "-> (body (25,3), face (70,3), hand (42,3))"
        v = _verts(smpl_mesh)
        return self.body25_reg.dot(v), self.face_reg.dot(v), self.hand_reg.dot(v)

    def get_body_kpts(self, smpl_mesh):
        "all 25 body keypoints"
        return self.body25_reg.dot(_verts(smpl_mesh))

    def get_smpl_center(self, smpl_mesh):
        return self.get_body_kpts(smpl_mesh)[8]

    def load_parts_ind(self, p="assets/smpl_parts_dense.pkl"):
        "part name -> vertex indices, in the file's dictionary order"
        with open(p, "rb") as f:
            return pkl.load(f)

    def get_part_verts(self, smpl, part_name):
        "smpl: (6890,3) vertices -> a copy of the vertices of the named part"
        return smpl[self.parts_inds[part_name]].copy()
