"""3-D median filter with the reference plugin's signature
(plugins/median_filter.py): `plugin -f median_filter --args "size=(3,1,1)"`.
The default size is the z-median that bridges a damaged or missing section.
Device chunks run the gfx950 kernels and stay on the device
(chunkflow_amd/filters.py)."""
from chunkflow_amd.filters import median_filter


def execute(chunk, size: tuple = (3, 1, 1), mode: str = 'reflect'):
    return [median_filter(chunk, size=size, mode=mode)]
