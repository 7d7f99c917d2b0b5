#!/usr/bin/env python3
"""Dev harness (not product): what a pitched device source costs the stage.

C2 geometry (u16 2048 x 2048 frames, 5-level pyramid, 256 x 256 chunks, 512
device-resident frames per launch), each row timed twice with HIP events on the
stage's stream (timing marks) after a warm-up launch:

  (a) contiguous frames, aqz_stage_append
  (b) rows pitched by 128 bytes (4096 + 128), read in place    direct route
  (c) a 2048 x 2048 ROI of a 2304 x 2304 canvas, read in place direct route
  (d) rows pitched by 2 bytes (4096 + 2)                       packed route

A launch is one append of 512 frames from a 512-frame source of random bytes
(4 GiB for (a), 5.1 GiB for the canvases of (c)), allocated per row, sized to
the last byte of the last row and freed after the row.

--pkg DIR runs another build (DIR holds its aqz package and libaqz_gpu.so),
e.g. the parent commit's for row (a): the yardstick is that build's row (a)
interleaved with this build's rows on the same box in one job, and the margin
is the spread of its own repeats.  One JSON line per row and repeat:

  python3 tools/strided_rate.py [--rows a,b,c,d] [--pkg DIR] [--label new]
                                [--out profiles/r12_strided_rate.jsonl]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIDE, CANVAS, FRAMES, BPP = 2048, 2304, 512, 2
ROW = SIDE * BPP


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="a,b,c,d")
    ap.add_argument("--pkg", default=os.path.join(REPO, "acquire-zarr_amd"))
    ap.add_argument("--label", default="new")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r12_strided_rate.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.pkg))
    import aqz
    import torch

    dev = torch.device("cuda", 0)
    dims = [(aqz.TIME, 0, 64, 1), (aqz.SPACE, SIDE, 256, 1), (aqz.SPACE, SIDE, 256, 1)]
    # (offset of pixel (0, 0), row stride, frame stride) in bytes
    layouts = {
        "a": (0, ROW, ROW * SIDE),
        "b": (0, ROW + 128, (ROW + 128) * SIDE),
        "c": (128 * CANVAS * BPP + 128 * BPP, CANVAS * BPP, CANVAS * CANVAS * BPP),
        "d": (0, ROW + 2, (ROW + 2) * SIDE),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for r in args.rows.split(","):
        off0, rs, fs = layouts[r]
        size = off0 + (FRAMES - 1) * fs + (SIDE - 1) * rs + ROW
        g = torch.Generator(device=dev)
        g.manual_seed(5)
        src = torch.randint(0, 256, (size,), dtype=torch.uint8, device=dev, generator=g)
        st = aqz.Stage(dims, aqz.UINT16, aqz.MEAN, force_levels=5, max_batch_frames=FRAMES,
                       layer_slots=8, device=0)
        ptr = src.data_ptr() + off0

        def launch():
            if r == "a":
                st.append_ptr(ptr, FRAMES, aqz.MEM_DEVICE)
            else:
                st.append_strided(ptr, FRAMES, rs, fs, aqz.MEM_DEVICE)

        launch()  # warm-up (allocates the packed route's buffer too)
        st.synchronize()
        for rep in range(args.repeats):
            st.timing_mark(0)
            launch()
            st.timing_mark(1)
            ms = st.timing_elapsed()
            st.synchronize()
            row = {"tool": "tools/strided_rate.py", "build": args.label, "row": r, "repeat": rep,
                   "row_stride": rs, "frame_stride": fs, "frames": FRAMES,
                   "ms_per_launch": round(ms, 3),
                   "input_gbs": round(FRAMES * ROW * SIDE / ms / 1e6, 1),
                   "kernel": st.dominant_kernel()}
            if hasattr(st, "source_report"):
                row["direct_frames"], row["packed_frames"] = st.source_report()
            row["device_bytes"] = st.memory_usage()["device_bytes"]
            print(json.dumps(row), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(row) + "\n")
        st.close()
        del src
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
