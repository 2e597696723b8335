"""Generates tests/golden/gridmap_obstacle.npz: the reference's map image gridmap.png as src/test/demo.cpp:98-107 reads it
(cv::imread(..., CV_8UC1): grayscale; addLayerFromImage with OCCUPY = 0, FREE = 255 keeps the bytes as they are), 701 x 710 cells,
values {0, 255}, obstacle where 0.  Stored in the C ABI's column-major layout [cols][rows] (the image transposed), bit-packed (np.packbits
of grid != 0) so that the tests need no image library.
Run from the repo root:  python tests/golden/make_distance_golden.py <the reference's gridmap.png>"""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))


def main(png):
    img = np.asarray(Image.open(png).convert("L"))          # ITU-R 601 luma, as OpenCV's grayscale read; alpha dropped
    assert set(np.unique(img).tolist()) <= {0, 255}, np.unique(img)
    rows, cols = img.shape                                  # grid_map size = (image rows, image cols)
    cm = np.ascontiguousarray(img.T)                        # [cols][rows]
    np.savez_compressed(os.path.join(HERE, "gridmap_obstacle.npz"), free_bits=np.packbits(cm.ravel() != 0), rows=rows, cols=cols,
                        resolution=0.2)
    print(f"gridmap_obstacle.npz: {rows} x {cols}, {int((img == 0).sum())} obstacle cells")


if __name__ == "__main__":
    main(sys.argv[1])
