"""CPU: chore_amd.render.look against what the reference's own look.py computes (tests/golden/look.npz, written by
tests/golden/make_look_golden.py).  Allowed: 4 x the fixture's `bound_<case>`, the largest difference between the reference's
float32 result and the same formula in float64."""
import numpy as np
import pytest
import torch

from conftest import golden


@pytest.mark.parametrize("name", ["default_up", "oblique", "batched"])
def test_look_against_the_reference(name):
    from chore_amd.render import look
    g = golden("look.npz")
    v = torch.from_numpy(g["vertices"])
    eye, direction, up = (torch.from_numpy(g["%s_%s" % (k, name)]) for k in ("eye", "direction", "up"))
    bound = 4 * float(g["bound_" + name])
    assert 0 < bound < 1e-5
    got = look(v, eye, direction, up)
    assert got.dtype == torch.float32 and np.abs(got.numpy() - g["out_" + name]).max() <= bound
    if eye.dim() == 1:                                  # lists and tuples, as the reference accepts them
        again = look(v, eye.tolist(), tuple(direction.tolist()), up.tolist())
        assert np.abs(again.numpy() - g["out_" + name]).max() <= bound
    if name == "default_up":
        assert torch.equal(look(v, eye, direction), got)


def test_look_is_differentiable_and_checks_its_input():
    from chore_amd.render import look
    v = torch.randn(2, 5, 3, requires_grad=True)
    look(v, [0.0, 0.0, -2.0], [0.0, 0.0, 1.0]).sum().backward()
    assert torch.isfinite(v.grad).all() and v.grad.abs().max() > 0
    with pytest.raises(ValueError):
        look(torch.zeros(5, 3), [0.0, 0.0, -2.0])
