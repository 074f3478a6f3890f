"""Per-section 2-D gaussian blur with the reference plugin's signature
(plugins/gaussian_filter.py): `plugin -f gaussian_filter --args "sigma=2"`.
A (C,z,y,x) chunk is filtered per channel. Device chunks run the gfx950
kernel and stay on the device (chunkflow_amd/filters.py)."""
from chunkflow_amd.filters import gaussian_filter_2d


def execute(chunk, sigma: float = 1., inplace=False):
    return gaussian_filter_2d(chunk, sigma=sigma, inplace=inplace)
