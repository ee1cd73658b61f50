"""Training-data preparation on the GPU: the exact point-to-mesh distance, the boundary sampler built on it, and the masks of a
frame from its meshes; the exact Euclidean distance transform of images."""
from .edt import distance_transform_edt  # noqa: F401
from .mesh_distance import mesh_distance  # noqa: F401
from .boundary_sampler import BoundarySampler, sample_surface  # noqa: F401
from .masks import frame_rows, render_masks  # noqa: F401
