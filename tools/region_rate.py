#!/usr/bin/env python3
"""Dev harness (not product): rates of region reads (aqz_reader_load_frames_region,
aqz_reader_read_region) over the layer of tools/read_rate.py: C2 level 0, 512 MiB
of camera-like u16, 64 frames of 2048 x 2048 in 64 chunks of 256x256x64 (8 MiB).

One process per JSON line, HIP events on the calling stream, --reps calls after a
warm-up call:

  (i)  read_region with the full frame as region, against read_frames of the same
       64 frames.  read_frames is timed twice back to back; the spread of those
       two runs is the margin read_region is held against.
  (ii) load_frames_region + read_region of a 512 x 512 crop of one frame, at a
       chunk-aligned origin (256, 256: 4 of the 64 chunks) and at (129, 131: 9 of
       64), against the only way to that crop without them: load_frames +
       read_frames of the layer.  --codec lz4: blosc-lz4 with the byte shuffle;
       --codec zstd: plain zstd, decoded with AQZ_DECODE_ZSTD_PARALLEL.  Reported
       as a ratio of times next to the ratio of chunks decoded.

  --window adds, in the same process, beside every load_frames_region + read_region
  row: load_frames_window + read_region of the same crop (decoding only the blosc blocks
  the crop's byte hull meets), and a window equal to the whole layer beside the region
  load of the whole layer.  Each row is timed twice; the spread of the region row's two
  runs is the margin.  Every line carries load_stats (decoded bytes, copied bytes).
  --codec blosc-zstd (blosc-zstd with the byte shuffle) is for this mode.

  python3 tools/region_rate.py --codec lz4 [--reps 20] [--out profiles/r10_region_rate.jsonl]
  python3 tools/region_rate.py --window --codec lz4|blosc-zstd|zstd \
      --out profiles/r11_window_rate.jsonl
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "acquire-zarr_amd"))

import aqz  # noqa: E402
import torch  # noqa: E402

N_CHUNKS, CHUNK = 64, 256 * 256 * 64 * 2
SIDE, PLANES = 2048, 64
DIMS = [(aqz.TIME, 0, PLANES, 1), (aqz.SPACE, SIDE, 256, 1), (aqz.SPACE, SIDE, 256, 1)]
CROP = 512
FRAME = 31                                  # the frame the crops are taken from


def camera(dev):
    n_px = N_CHUNKS * CHUNK // 2
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x = torch.arange(n_px, device=dev, dtype=torch.float32)
    v = 1000.0 + 200.0 * torch.sin(x / 977.0) + 30.0 * torch.randn(n_px, device=dev, generator=g)
    return v.clamp(0, 65535).to(torch.int32).to(torch.int16).view(torch.uint8)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--codec", choices=("lz4", "blosc-zstd", "zstd"), default="lz4")
    ap.add_argument("--window", action="store_true",
                    help="time load_frames_window beside every load_frames_region row")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r10_region_rate.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    layer_bytes = N_CHUNKS * CHUNK
    frame_bytes = SIDE * SIDE * 2

    frames = camera(dev)
    st = aqz.Stage(DIMS, aqz.UINT16, aqz.MEAN, multiscale=False, layer_slots=1,
                   max_batch_frames=PLANES)
    st.append_ptr(frames.data_ptr(), PLANES, aqz.MEM_DEVICE)
    st.synchronize()
    chunks, flags, tag = st.device_layer(0, 0)
    pitch = st.layout(0)["chunk_pitch"]
    out = torch.empty(layer_bytes, dtype=torch.uint8, device=dev)
    images = frames.view(torch.int16).view(PLANES, SIDE, SIDE)

    if args.codec == "lz4":
        code, codecs, shuffle = aqz.CODEC_BLOSC_LZ4, aqz.DECODE_CODEC_LZ4, 1
    elif args.codec == "blosc-zstd":
        code, codecs, shuffle = aqz.CODEC_BLOSC_ZSTD, aqz.DECODE_CODEC_ZSTD, 1
    else:
        code, shuffle = aqz.CODEC_ZSTD, 0
        codecs = aqz.DECODE_CODEC_ZSTD | aqz.DECODE_ZSTD_PARALLEL
    rd = aqz.Reader(DIMS, aqz.UINT16, codecs=codecs)
    row = {"tool": "tools/region_rate.py", "codec": args.codec,
           "layer": "C2 level 0: 64 frames of 2048x2048 u16 in 64 chunks of 256x256x64",
           "layer_bytes": layer_bytes, "reps": args.reps}

    # (i) the full frame as a region against read_frames, the layer loaded once
    whole = (0, 0, SIDE, SIDE)
    rd.load_chunks(chunks, pitch, flags, tag, stream)
    read_frames = lambda: rd.read_frames_ptr(0, PLANES, out.data_ptr(), frame_bytes, stream)
    read_region = lambda: rd.read_region_ptr(0, PLANES, whole, out.data_ptr(), SIDE * 2,
                                             frame_bytes, stream)
    f1 = timed(read_frames, args.reps)
    f2 = timed(read_frames, args.reps)
    out.zero_()
    r1 = timed(read_region, args.reps)
    exact = bool(torch.equal(out, frames))
    r2 = timed(read_region, args.reps)
    row.update({"read_frames_ms": [round(f1, 4), round(f2, 4)],
                "read_region_whole_ms": [round(r1, 4), round(r2, 4)],
                "read_frames_spread": round(abs(f1 - f2) / min(f1, f2), 4),
                "read_region_over_read_frames": round(min(r1, r2) / min(f1, f2), 4),
                "read_region_whole_exact": exact})

    # (ii) a 512 x 512 crop of one frame against the full load + read
    st.compress_layer(0, 0, codec=code, clevel=5 if args.codec == "lz4" else 3, shuffle=shuffle)
    off = st.compressed_offsets(0, 0)
    total = int(off[-1])
    cfr = torch.empty(total, dtype=torch.uint8, device=dev)
    st.copy_compressed_async(0, 0, cfr.data_ptr(), total)
    st.wait_copies()
    out.zero_()

    def full():
        rd.load_frames(cfr, off, None, code, frames_bytes=total, stream_ptr=stream)
        rd.read_frames_ptr(0, PLANES, out.data_ptr(), frame_bytes, stream)

    full_ms = timed(full, args.reps)
    _, bad = rd.status()
    row.update({"compressed_bytes": total, "full_ms": round(full_ms, 3),
                "full_exact": bool(torch.equal(out, frames)) and bad == 0,
                "full_load_stats": list(rd.load_stats())})
    crop = torch.empty(CROP * CROP * 2, dtype=torch.uint8, device=dev)
    for key, (x0, y0) in (("aligned", (256, 256)), ("unaligned", (129, 131))):
        region = (x0, y0, CROP, CROP)
        n_need = len(rd.region_chunks(FRAME, 1, region))
        crop.zero_()

        def crop_read():
            rd.load_frames_region(cfr, off, FRAME, 1, region, None, code, frames_bytes=total,
                                  stream_ptr=stream)
            rd.read_region_ptr(FRAME, 1, region, crop.data_ptr(), CROP * 2, CROP * CROP * 2,
                               stream)

        ms = timed(crop_read, args.reps)
        _, bad = rd.status()
        want = images[FRAME, y0:y0 + CROP, x0:x0 + CROP].contiguous().view(torch.uint8).flatten()
        if args.window:
            # the same crop through the window load, the region row timed again beside it
            def window_read():
                rd.load_frames_window(cfr, off, FRAME, 1, region, None, code,
                                      frames_bytes=total, stream_ptr=stream)
                rd.read_region_ptr(FRAME, 1, region, crop.data_ptr(), CROP * 2,
                                   CROP * CROP * 2, stream)

            region_stats = list(rd.load_stats())
            ms2 = timed(crop_read, args.reps)
            crop.zero_()
            w1 = timed(window_read, args.reps)
            _, wbad = rd.status()
            w_exact = bool(torch.equal(crop, want)) and wbad == 0
            w_stats = list(rd.load_stats())
            w2 = timed(window_read, args.reps)
            row.update({key + "_region_ms": [round(ms, 4), round(ms2, 4)],
                        key + "_window_ms": [round(w1, 4), round(w2, 4)],
                        key + "_region_spread": round(abs(ms - ms2) / min(ms, ms2), 4),
                        key + "_window_over_region": round(min(w1, w2) / min(ms, ms2), 4),
                        key + "_region_load_stats": region_stats,
                        key + "_window_load_stats": w_stats,
                        key + "_window_exact": w_exact})
            crop.zero_()
            crop_read()
            torch.cuda.synchronize()
        row.update({key + "_origin": [x0, y0], key + "_chunks": n_need,
                    key + "_ms": round(ms, 4),
                    key + "_time_ratio": round(ms / full_ms, 4),
                    key + "_chunk_ratio": round(n_need / N_CHUNKS, 4),
                    key + "_exact": bool(torch.equal(crop, want)) and bad == 0})
    if args.window:
        # a window equal to the whole layer beside the region load of the whole layer
        def whole_read(window):
            load = rd.load_frames_window if window else rd.load_frames_region
            load(cfr, off, 0, PLANES, whole, None, code, frames_bytes=total, stream_ptr=stream)
            rd.read_region_ptr(0, PLANES, whole, out.data_ptr(), SIDE * 2, frame_bytes, stream)

        g1 = timed(lambda: whole_read(False), args.reps)
        g_stats = list(rd.load_stats())
        g2 = timed(lambda: whole_read(False), args.reps)
        out.zero_()
        w1 = timed(lambda: whole_read(True), args.reps)
        _, wbad = rd.status()
        w_exact = bool(torch.equal(out, frames)) and wbad == 0
        w_stats = list(rd.load_stats())
        w2 = timed(lambda: whole_read(True), args.reps)
        row.update({"whole_region_ms": [round(g1, 3), round(g2, 3)],
                    "whole_window_ms": [round(w1, 3), round(w2, 3)],
                    "whole_region_spread": round(abs(g1 - g2) / min(g1, g2), 4),
                    "whole_window_over_region": round(min(w1, w2) / min(g1, g2), 4),
                    "whole_region_load_stats": g_stats, "whole_window_load_stats": w_stats,
                    "whole_window_exact": w_exact})
    rd.close()
    st.close()
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
