"""Plugin `agglomerate`: affinity map in, segmentation out.

Same call signature as the reference's plugin of this name, so its command
line runs unchanged:

    plugin -f agglomerate -i affs -o seg --args "threshold=0.7;..."

The reference hands the work to the waterz wheel; here it is
chunkflow_amd.watershed (watershed fragments, region graph and mean-affinity
agglomeration; gfx950 kernels when the chunk is on the device, where the
result stays). DESIGN.md, "Watershed and agglomeration", says where the
result knowingly differs from waterz's.
"""
import numpy as np

from chunkflow_amd.chunk import Chunk
from chunkflow_amd.watershed import agglomerate

# waterz's default: merge while 1 - mean affinity < threshold
MEAN_AFFINITY = 'OneMinus<MeanAffinity<RegionGraphType, ScoreValue>>'


def execute(affs: Chunk,
            fragments: np.ndarray = None,
            threshold: float = 0.7,
            aff_threshold_low: float = 0.001,
            aff_threshold_high: float = 0.9999,
            scoring_function: str = MEAN_AFFINITY,
            flip_channel: bool = True):
    """affs: (3, z, y, x) in chunkflow's channel order x, y, z; with
    flip_channel=False it is in z, y, x order already and is flipped back
    here. Returns [segmentation chunk] with the input's voxel offset and
    voxel size."""
    if scoring_function.replace(' ', '') != MEAN_AFFINITY.replace(' ', ''):
        raise ValueError(
            f'agglomerate: unsupported scoring_function '
            f'{scoring_function!r}; the one that is supported is '
            f'{MEAN_AFFINITY!r}')
    if not isinstance(affs, Chunk):
        affs = Chunk(affs)
    if not flip_channel:
        flipped = (affs.array.flip(0) if affs.is_device
                   else np.flip(np.asarray(affs.array), axis=0))
        affs = Chunk(flipped, voxel_offset=affs.voxel_offset,
                     voxel_size=affs.voxel_size)
    # 1 - mean < threshold  <=>  mean > 1 - threshold
    seg = agglomerate(affs, 1.0 - threshold, aff_threshold_low,
                      aff_threshold_high, fragments=fragments)
    return [seg]
