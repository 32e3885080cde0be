#!/usr/bin/env python3
"""Records tests/golden/plan_sizes.json: what the C-ABI shows of a launch's
shape (tile grid, batch limit, workspace sizes and the answers to batches past
the limits) over a table of frames and batch sizes. tests/plan_table.py has the
format and the calls; tests/test_plan_table.py replays them against the built
library.

TEST INFRASTRUCTURE ONLY. The table pins one revision's arithmetic, so it is
recorded from that revision's library and then must be reproduced by every
later one:

    bash tools/build_ref_variant.sh <rev> parent
    PTMI_LIB=path-tracer-python_amd/ptmi/_lib/variants/libptmi_parent.so \\
        python tests/golden/gen_plan_sizes.py

(PTMI_LIB unset: the in-tree library; ``--check`` compares with the committed
file and writes nothing.) It was recorded from the last revision whose
launchers derived tiles, limits and layouts themselves. No call in it reaches
the HIP runtime.

The frames are those of csrc/plan_check.cpp: tiny and ragged ones, an 800 x 800
frame whole, windowed and in four band partitions (band_rows, band_stride,
band_offset), and a 4K frame; the batches 1 .. 1024, each frame's own
ptmi_mk_max_batch and one more, and the rejected 0 and -1.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, 'path-tracer-python_amd'), os.path.join(ROOT, 'tests')]

import plan_table  # noqa: E402
from ptmi import _lib  # noqa: E402

BATCHES = [1, 2, 3, 4, 5, 16, 64, 1024, 0, -1]


def whole(width, height, **more):
    return dict(dict(width=width, height=height, w=width, h=height, band_rows=1, band_stride=1, max_depth=50), **more)


FRAMES = [whole(1, 1), whole(3, 1), whole(13, 7), whole(64, 64), whole(800, 800),
          whole(800, 800, x0=397, y0=301, w=5, h=3)]
FRAMES += [whole(800, 800, band_rows=r, band_stride=s, band_offset=o)
           for r, s, o in ((4, 8, 3), (2, 4, 1), (1, 8, 0), (8, 3, 2))]
FRAMES.append(whole(3840, 2160))


def record():
    lib = _lib.load()
    cases = [plan_table.answer(lib, {k: v for k, v in f.items() if v != 0}, BATCHES) for f in FRAMES]
    return '[\n' + ',\n'.join(json.dumps(c) for c in cases) + '\n]\n'


if __name__ == '__main__':
    text = record()
    if '--check' in sys.argv:
        with open(plan_table.TABLE) as f:
            same = f.read() == text
        print('identical' if same else 'DIFFERENT', plan_table.TABLE)
        sys.exit(0 if same else 1)
    with open(plan_table.TABLE, 'w') as f:
        f.write(text)
    print(f'{text.count(chr(10)) - 2} frames -> {plan_table.TABLE}')
