from .image_prep import ImagePrep  # noqa: F401
from .train_image_prep import TrainImagePrep  # noqa: F401
