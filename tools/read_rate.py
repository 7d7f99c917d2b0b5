#!/usr/bin/env python3
"""Dev harness (not product): rates of the device reader (aqz_reader_*) over one
C2-shaped level-0 chunk layer: 512 MiB of camera-like u16, 64 frames of
2048 x 2048 in 64 chunks of 256x256x64 (8 MiB).

Three paths, each timed with HIP events on the stream it is enqueued on, in
this one process, after a warm-up call:

  (a) read_frames of the whole layer after one       the un-split kernel alone;
      load_chunks; and load_chunks + read_frames     with the load in the window
  (b) load_frames + read_frames, blosc-lz4 with      the decoder, then the
      byte shuffle and with bitshuffle               un-split kernel
  (c) aqz_probe_hbm, shape copy (1 read : 1 write)   the plain copy probe over
                                                     as many bytes, same box

(a) is reported as a fraction of (c): boxes differ by up to 12 %, so the probe
of the same process is the yardstick, never a fixed number.  Rates are GB/s
(1e9) of frame bytes written (= chunk bytes read).  One JSON line per run:

  python3 tools/read_rate.py [--reps 20] [--out profiles/r08_read_rate.jsonl]
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r08_read_rate.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    layer_bytes = N_CHUNKS * CHUNK
    frame_bytes = SIDE * SIDE * 2
    gbs = lambda ms: round(layer_bytes / ms / 1e6, 1)

    # the layer: frames through a stage, so the chunks are what the product writes
    frames = camera(dev)
    st = aqz.Stage(DIMS, aqz.UINT16, aqz.MEAN, multiscale=False, layer_slots=1,
                   max_batch_frames=PLANES)
    st.append_ptr(frames.data_ptr(), PLANES, aqz.MEM_DEVICE)
    st.synchronize()
    chunks, flags, tag = st.device_layer(0, 0)
    pitch = st.layout(0)["chunk_pitch"]
    out = torch.empty(layer_bytes, dtype=torch.uint8, device=dev)

    rd = aqz.Reader(DIMS, aqz.UINT16, codecs=aqz.DECODE_CODEC_LZ4)
    row = {"tool": "tools/read_rate.py",
           "layer": "C2 level 0: 64 frames of 2048x2048 u16 in 64 chunks of 256x256x64",
           "layer_bytes": layer_bytes, "reps": args.reps,
           "reader_device_bytes": rd.device_bytes()}

    def unsplit():
        rd.load_chunks(chunks, pitch, flags, tag, stream)
        rd.read_frames_ptr(0, PLANES, out.data_ptr(), frame_bytes, stream)

    # the kernel alone (the layer stays loaded), then with the load in the window
    unsplit()
    a_ms = timed(lambda: rd.read_frames_ptr(0, PLANES, out.data_ptr(), frame_bytes, stream),
                 args.reps)
    al_ms = timed(unsplit, args.reps)
    row.update({"unsplit_ms": round(a_ms, 3), "unsplit_gbs": gbs(a_ms),
                "load_chunks_unsplit_ms": round(al_ms, 3),
                "load_chunks_unsplit_gbs": gbs(al_ms),
                "unsplit_exact": bool(torch.equal(out, frames))})

    for shuffle, key in ((1, "lz4_shuffle"), (2, "lz4_bitshuffle")):
        st.compress_layer(0, 0, codec=aqz.CODEC_BLOSC_LZ4, clevel=5, shuffle=shuffle)
        off = st.compressed_offsets(0, 0)
        total = int(off[-1])
        cfr = torch.empty(total, dtype=torch.uint8, device=dev)
        st.copy_compressed_async(0, 0, cfr.data_ptr(), total)
        st.wait_copies()
        out.zero_()

        def decode_and_unsplit():
            rd.load_frames(cfr, off, None, aqz.CODEC_BLOSC_LZ4, frames_bytes=total,
                           stream_ptr=stream)
            rd.read_frames_ptr(0, PLANES, out.data_ptr(), frame_bytes, stream)

        b_ms = timed(decode_and_unsplit, args.reps)
        status, bad = rd.status()
        row.update({key + "_ms": round(b_ms, 3), key + "_gbs": gbs(b_ms),
                    key + "_ratio": round(layer_bytes / total, 3),
                    key + "_exact": bool(torch.equal(out, frames)) and bad == 0})
    rd.close()
    st.close()

    # the copy probe last, as decode_rate.py's compressor: same process, same box
    c_ms, c_read = aqz.probe_hbm(aqz.PROBE_COPY, nbytes=layer_bytes, reps=args.reps)
    row.update({"copy_probe_ms": round(c_ms, 3), "copy_probe_read_bytes": int(c_read),
                "copy_probe_gbs": round(c_read / c_ms / 1e6, 1),
                "unsplit_over_copy_probe": round((layer_bytes / a_ms) / (c_read / c_ms), 3)})
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
