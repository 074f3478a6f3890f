"""Build the in-tree HIP extension (gfx950)."""
import os
import subprocess

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(PKG_DIR, 'libchunkflow_amd.so')
CSRC = os.path.join(PKG_DIR, 'csrc')
# the translation units, in the order of the hipcc line, and what they include
SOURCES = [os.path.join(CSRC, name + '.hip')
           for name in ('cfx', 'cc', 'image', 'conv', 'updown', 'downsample',
                        'labels', 'watershed', 'filter')]
HEADERS = [os.path.join(CSRC, 'cfx_internal.h'),
           os.path.join(CSRC, 'cc_unionfind.h'),
           os.path.join(CSRC, 'label_table.h'),
           os.path.join(PKG_DIR, '..', 'include', 'chunkflow_amd.h')]


def so_is_fresh() -> bool:
    if not os.path.exists(SO_PATH):
        return False
    so_mtime = os.path.getmtime(SO_PATH)
    return all(os.path.getmtime(p) <= so_mtime for p in SOURCES + HEADERS)


def build(force: bool = False) -> str:
    """Compile chunkflow_amd/csrc/*.hip -> libchunkflow_amd.so in-tree.

    hipcc cross-compiles for gfx950 without a GPU; the .so ships to the GPU
    box inside the repo snapshot.
    """
    if not force and so_is_fresh():
        return SO_PATH
    cmd = [
        'hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17',
        '-ffp-contract=off', '-fPIC', '-shared', *SOURCES, '-o', SO_PATH,
    ]
    subprocess.run(cmd, check=True)
    return SO_PATH


if __name__ == '__main__':
    print(build(force=True))
