"""csrc/device/tile_layout.hpp is THE definition of the pixel-tile shard for host and device code: which 32x32 blocks a rank owns and where local pixel L of
its block-major buffers lies in the image.  It needs no HIP, so a small driver compiled with g++ prints for_each_local_pixel over owned_blocks, checked here
against the numpy definitions of adypt_amd/distributed.py (owner_mask, tile_from_image), which share no expression with the header."""
import os
import subprocess

import numpy as np
import pytest

from adypt_amd import distributed

DEVICE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adypt_amd", "csrc", "device")
DRIVER = r"""
#include "tile_layout.hpp"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv)
{
	if(argc != 5) return 1;
	const int w = atoi(argv[1]), h = atoi(argv[2]), rank = atoi(argv[3]), nranks = atoi(argv[4]);
	const std::vector<int32_t> blocks = adypt::owned_blocks(w, h, rank, nranks);
	printf("%zu\n", blocks.size());
	adypt::for_each_local_pixel(blocks, w, h, [](size_t L, int x, int y) { printf("%zu %d %d\n", L, x, y); });
	return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("tile_layout")
    (d / "driver.cpp").write_text(DRIVER)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + DEVICE, str(d / "driver.cpp"), "-o", str(d / "driver")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]  # (also: the header needs neither hipcc nor a HIP include)
    return str(d / "driver")


@pytest.mark.parametrize("w,h", [(96, 64), (100, 75), (33, 31), (1, 1), (64, 36), (257, 40)])
@pytest.mark.parametrize("world", [1, 2, 3, 4, 8])
def test_local_pixels_are_where_numpy_puts_them(driver, w, h, world):
    image = np.zeros((h, w, 4), dtype=np.float32)
    image[..., 0] = np.arange(1, w * h + 1, dtype=np.float32).reshape(h, w)  # pixel (x, y) holds y * w + x + 1; 0 = padding of a block that sticks out
    seen = np.zeros((h, w), dtype=np.int32)
    for rank in range(world):
        lines = subprocess.run([driver, str(w), str(h), str(rank), str(world)], stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")
        local = distributed.tile_from_image(image, rank, world)
        assert int(lines[0]) * 1024 == local.shape[0]
        px = np.array([list(map(int, ln.split())) for ln in lines[1:] if ln], dtype=np.int64).reshape(-1, 3)
        L, x, y = px[:, 0], px[:, 1], px[:, 2]
        assert np.array_equal(local[L, 0], (y * w + x + 1).astype(np.float32))
        assert len(L) == np.count_nonzero(local[:, 0]) and len(np.unique(L)) == len(L)  # every local pixel inside the image, once
        mask = np.zeros((h, w), dtype=np.uint8)
        mask[y, x] = 1
        assert np.array_equal(mask, distributed.owner_mask(w, h, rank, world))
        seen[y, x] += 1
    assert np.all(seen == 1)
