from sleap_nn_amd.data.augmentation import (  # noqa: F401
    Augmenter,
    apply_flip_augmentation,
    apply_geometric_augmentation,
    apply_intensity_augmentation,
)
from sleap_nn_amd.data.tiling import generate_tile_grid  # noqa: F401
from sleap_nn_amd.data.targets import (  # noqa: F401
    TargetGenerator,
    filter_oob_points,
    generate_centroids,
    generate_class_maps,
    generate_confmaps,
    generate_multiconfmaps,
    generate_pafs,
    make_class_vectors,
)
