"""The masks of a frame from its registered meshes: what BEHAVE ships per frame as k*.person_mask, k*.obj_rend_mask (the object
as seen, occluded by the person) and k*.obj_rend_full (the object alone), plus the body alone.

One instances call (chore_instances_fwd) through the Kinect colour camera of utils/render_utils.setup_renderer; the frame is
the upper `height * image_size / width` rows of the square rendering.  The arrays feed TrainImagePrep.prepare(rgb, person_mask,
obj_mask) as they are.  Reading and writing the dataset's mask files stays with the caller."""
import numpy as np

MASK_THRESHOLD = 0.5        # coverage of a pixel (the mean over its 2 x 2 samples) from which it counts as covered


def frame_rows(image_size, height=1536, width=2048):
    """rows of a square `image_size` rendering that the height x width frame takes: its upper height * image_size / width"""
    image_size, height, width = int(image_size), int(height), int(width)
    if image_size <= 0 or height <= 0 or width <= 0 or height > width:
        raise ValueError("a frame no higher than wide and a positive image_size expected, got %d x %d at %d"
                         % (width, height, image_size))
    return height * image_size // width


def render_masks(smpl_mesh, obj_mesh, image_size=2048, height=1536, width=2048, device="cuda:0"):
    """meshes with .v (camera coordinates of the Kinect colour camera) / .f -> dict of uint8 (rows, image_size) arrays, 255 where
    the coverage is >= 0.5: person_mask / obj_rend_mask (each mesh where the other is not in front), person_full / obj_rend_full
    (each mesh alone).  rows = frame_rows(image_size, height, width)."""
    from ..utils.render_utils import NrWrapper
    rows = frame_rows(image_size, height, width)
    wrapper = NrWrapper(device=device, image_size=image_size)
    wrapper.front_renderer.anti_aliasing = True
    visible, full, _ = wrapper.render_masks(wrapper.front_renderer, [smpl_mesh, obj_mesh])
    as_u8 = lambda cov: ((cov[:rows] >= MASK_THRESHOLD).byte() * 255).cpu().numpy()      # noqa: E731
    return {"person_mask": as_u8(visible[0]), "person_full": as_u8(full[0]),
            "obj_rend_mask": as_u8(visible[1]), "obj_rend_full": as_u8(full[1])}
