"""Grids and binary patterns shared by the object-cell tests (tests/test_objects_cpu.py, tests/test_gpu_objects.py): the host
build of the labelling pieces runs over the same maps as the kernels."""
import numpy as np

# (n_y, n_x): one cell; one row and one column of the longest grid; the smallest grid with both axes; rows and columns that cross
# the 64-lane chunks at non-multiples of 64, once and twice
SHAPES = [(1, 1), (1, 1023), (1023, 1), (2, 3), (65, 67), (130, 5), (5, 130)]

PATTERNS = ('full', 'run', 'checkerboard', 'diagonal', 'antidiagonal', 'comb', 'serpentine', 'spiral')


def pattern(name, shape):
    """A bool map [n_y, n_x]."""
    n_y, n_x = shape
    yy, xx = np.indices(shape)
    b = np.zeros(shape, dtype=bool)
    if name == 'full':
        b[:] = True
    elif name == 'run':                           # single runs that cross every chunk border, one cell short at both ends
        b[::2, 1:max(n_x - 1, 2)] = True
    elif name == 'checkerboard':                  # 4: every cell an object; 8: one object
        b = (yy + xx) % 2 == 0
    elif name == 'diagonal':                      # 4: single cells; 8: lines that run down to the right
        b = (yy - xx) % 3 == 0
    elif name == 'antidiagonal':                  # ... and down to the left: the first cell is not the first one met in its row
        b = (yy + xx) % 3 == 0
    elif name == 'comb':                          # teeth that join only in the last row: the merges come late
        b[:, ::2] = True
        b[-1, :] = True
    elif name == 'serpentine':                    # one path through the whole grid: the root lies far along a long chain
        b[::2, :] = True
        for k, y in enumerate(range(1, n_y, 2)):
            b[y, -1 if k % 2 == 0 else 0] = True
    elif name == 'spiral':                        # a square spiral inward, walls two cells apart
        y0, y1, x0, x1 = 0, n_y - 1, 0, n_x - 1
        first = True
        while y0 <= y1 and x0 <= x1:
            b[y0, (x0 if first else max(x0 - 1, 0)):x1 + 1] = True
            b[y0:y1 + 1, x1] = True
            if y1 > y0:
                b[y1, x0:x1 + 1] = True
            if y1 - 1 > y0 + 1:
                b[y0 + 2:y1 + 1, x0] = True
            y0, y1, x0, x1, first = y0 + 2, y1 - 2, x0 + 2, x1 - 2, False
    else:
        raise ValueError(name)
    return b
