"""the names `import neural_renderer as nr` gives the reference's visualisation code (utils/render_utils.py)"""
from ..recon.obj_pose_roi import projection, vertices_to_faces  # noqa: F401
from .obj_io import create_texture_image, load_mtl, load_obj, load_textures, save_obj  # noqa: F401
from .renderer import (Renderer, face_light, face_visibility, get_points_from_angles, lighting, look, look_at,  # noqa: F401
                       perspective, photo_textures, point_visibility, rasterize_instances, rasterize_rgbad, rasterize_scene,
                       sample_depth, splat_points, world_radius_to_pixels)
