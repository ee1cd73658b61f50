"""Generate tests/golden/look.npz by running THE REFERENCE's own `look` (external/neural_renderer/neural_renderer/look.py)
on CPU tensors.

Run in the build container only (needs /root/reference):

    python tests/golden/make_look_golden.py

neural_renderer's package __init__ pulls in its CUDA extension and cannot be imported, so look.py is loaded by path (the
mechanism of make_render_golden.py).  Its default `up` is a CUDA tensor, so every call passes `up` explicitly; the default's
value, [0, 1, 0], is one of the recorded cases.  The fixture holds arrays only: seeded inputs, the reference's float32 results,
and `bound_<case>`, the largest difference between a result and the same formula evaluated in float64 by this script (the
test allows 4 x that).
"""
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LOOK_PY = "/root/reference/external/neural_renderer/neural_renderer/look.py"


def look64(v, eye, direction, up):
    def norm(a):
        return a / np.maximum(np.linalg.norm(a, axis=-1, keepdims=True), 1e-5)
    v, eye, direction, up = (np.asarray(a, np.float64) for a in (v, eye, direction, up))
    eye, direction, up = (a[None] if a.ndim == 1 else a for a in (eye, direction, up))
    z = norm(direction)
    x = norm(np.cross(up, z))
    y = norm(np.cross(z, x))
    r = np.stack([np.broadcast_to(a, (max(len(x), len(y), len(z)), 3)) for a in (x, y, z)], 1)
    return np.matmul(v - eye[:, None, :], r.transpose(0, 2, 1))


def main():
    spec = importlib.util.spec_from_file_location("reference_look", LOOK_PY)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rs = np.random.RandomState(0)
    B, V = 4, 17          # not 3: the reference calls torch.cross without `dim`, which takes the FIRST axis of size 3
    v = rs.uniform(-1, 1, (B, V, 3)).astype(np.float32)
    out = {"vertices": v}
    cases = {
        "default_up": (np.array([0.3, -0.2, -2.5], np.float32), np.array([0, 0, 1], np.float32), np.array([0, 1, 0], np.float32)),
        "oblique": (np.array([1.0, 0.5, -2.0], np.float32), np.array([-0.4, -0.1, 0.9], np.float32), np.array([0.1, 1, 0], np.float32)),
        "batched": (rs.uniform(-2, 2, (B, 3)).astype(np.float32), rs.standard_normal((B, 3)).astype(np.float32),
                    (np.array([0, 1, 0]) + 0.2 * rs.standard_normal((B, 3))).astype(np.float32)),
    }
    for name, (eye, direction, up) in cases.items():
        got = mod.look(torch.from_numpy(v), torch.from_numpy(eye), torch.from_numpy(direction), torch.from_numpy(up)).numpy()
        assert got.dtype == np.float32 and got.shape == v.shape
        out["eye_" + name], out["direction_" + name], out["up_" + name], out["out_" + name] = eye, direction, up, got
        out["bound_" + name] = np.float64(np.abs(got - look64(v, eye, direction, up)).max())
        print(name, "bound", out["bound_" + name])
    out["description"] = np.array("look.py:6-55 of the reference on CPU float32 tensors, `up` passed explicitly")
    np.savez_compressed(os.path.join(HERE, "look.npz"), **out)


if __name__ == "__main__":
    main()
