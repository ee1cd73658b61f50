"""Training-data preparation on the GPU: the exact point-to-mesh distance and the boundary sampler built on it."""
from .mesh_distance import mesh_distance  # noqa: F401
from .boundary_sampler import BoundarySampler, sample_surface  # noqa: F401
