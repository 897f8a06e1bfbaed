from sleap_nn_amd.data.augmentation import (  # noqa: F401
    Augmenter,
    apply_flip_augmentation,
    apply_geometric_augmentation,
    apply_intensity_augmentation,
)
from sleap_nn_amd.data.tiling import generate_tile_grid  # noqa: F401
