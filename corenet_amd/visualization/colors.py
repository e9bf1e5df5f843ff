"""The label colour palette of the visualisations (reference: visualization/colors.py)."""
import numpy as np

# label 0 (void) is negative: the voxel renderer skips voxels whose colour has a negative channel
_DEFAULT_INTEGER_COLOR_PALETTE = (
    (-255, -255, -255),
    (120, 120, 120), (180, 120, 120), (6, 230, 230), (80, 50, 50), (4, 200, 3), (120, 120, 80), (140, 140, 140),
    (204, 5, 255), (230, 230, 230), (4, 250, 7), (224, 5, 255), (235, 255, 7), (150, 5, 61), (120, 120, 70),
    (8, 255, 51), (255, 6, 82),
)

DEFAULT_COLOR_PALETTE = np.array(_DEFAULT_INTEGER_COLOR_PALETTE, np.float32) / 255.0
