"""The head of the lattice workgroups in scripts/wg_timing.py's records (diagnostic build; 100 MHz
stamps): per whole-frame case, the time from a workgroup's first stamp to thread 0's head stamp
(column 4: the tile's masks are in registers and the first closest-hit step is next; 0 for a
workgroup that left before it -- a black tile, or one outside the RGB24 window), the duration of
the full and of the black workgroups, and the sum of all durations.  Busy slots per CU:
scripts/wg_slots.py.  Usage: python scripts/wg_head.py DIR [DIR ...]"""
import glob
import os
import sys

import numpy as np

US = 0.01   # 100 MHz ticks -> us
for d in sys.argv[1:]:
    for f in sorted(glob.glob(os.path.join(d, "whole_*.npy"))):
        r = np.load(f).astype(np.int64)
        lt = r[((r[:, 0] >> 56) & 0xFF) == 2]
        dur = (lt[:, 2] - lt[:, 1]) * US
        full = lt[:, 4] != 0
        head = (lt[full, 4] - lt[full, 1]) * US
        blk = dur[~full]
        span = (lt[:, 2].max() - lt[:, 1].min()) * US
        print(f"{f}: {len(lt)} workgroups, span {span:.1f} us; full {full.sum()}: mean {dur[full].mean():.2f} median "
              f"{np.median(dur[full]):.2f} us, head mean {head.mean():.3f} median {np.median(head):.3f} p10 "
              f"{np.percentile(head, 10):.3f} p90 {np.percentile(head, 90):.3f} us; black {len(blk)}: mean {blk.mean():.2f} "
              f"median {np.median(blk):.2f} us; all durations {dur.sum():.0f} us")
