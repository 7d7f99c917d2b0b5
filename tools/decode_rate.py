#!/usr/bin/env python3
"""Dev harness (not product): rates of the device decoders (blosc1-LZ4; with
--codecs blosc-zstd,zstd also the zstd decoder) and of the stage's on-device
verification, next to the device compressor's rate on the same data and
c-blosc's (libzstd's, for plain zstd frames) one-core decode of the same
frames on this host.

One C2-shaped chunk layer: 512 MiB of camera-like u16 in 64 chunks of
256x256x64 (8 MiB), lz4 clevel 5, byte shuffle and bitshuffle.  Everything is
timed in this one process after a warm-up run of each call:

  aqz_compressor_run, aqz_decompressor_run   HIP events on the stream they are
                                             enqueued on, `--reps` calls each
  aqz_stage_verify_layer + _verify_result    the stage enqueues on its own
                                             hand-off stream, so a host clock
                                             around the pair (it ends in the
                                             wait of verify_result)
  c-blosc                                    blosc_decompress_ctx, one thread,
                                             over `--host-chunks` frames

Rates are GB/s (1e9) of uncompressed bytes.  One JSON line per shuffle mode:

  python3 tools/decode_rate.py [--reps 10] [--out profiles/r07_decode_rate.jsonl]
  python3 tools/decode_rate.py --codecs blosc-zstd,zstd --clevel 3 --out <file>

--zstd-parallel {on,both} measures the plain-zstd layer (AQZ_CODEC_ZSTD) with the
block-parallel decoder (AQZ_DECODE_ZSTD_PARALLEL) instead: `both` times, in this
one process and on the same frames, the serial decoder, the parallel decoder and
the stage verify of each, `--repetitions` times each and interleaved (serial,
parallel, serial, ...; one call per repetition), and libzstd on one core as often.
One JSON line with every repetition, the fastest and slowest of each, and the
condition the parallel path is held to: its slowest repetition above the serial
decoder's fastest and above libzstd's fastest one-core rate.

  python3 tools/decode_rate.py --zstd-parallel both --clevel 3 \
      --out profiles/r09_zstd_parallel_rate.jsonl
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "acquire-zarr_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import aqz  # noqa: E402
import torch  # noqa: E402

N_CHUNKS, CHUNK = 64, 256 * 256 * 64 * 2
SIDE, PLANES = 2048, 64          # 8 x 8 chunks of 256 x 256, 64 planes deep


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


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def zstd_parallel_row(args, dev, stream, src):
    """The plain-zstd layer through the serial and / or the parallel decoder."""
    from codec_helpers import libzstd, zstd_decode
    layer_bytes = N_CHUNKS * CHUNK
    gbs = lambda ms: round(layer_bytes / ms / 1e6, 2)
    modes = {"on": ["parallel"], "both": ["serial", "parallel"]}[args.zstd_parallel]
    mask = {"serial": aqz.DECODE_CODEC_ZSTD,
            "parallel": aqz.DECODE_CODEC_ZSTD | aqz.DECODE_ZSTD_PARALLEL}
    comp = aqz.Compressor(CHUNK, 2, codec=aqz.CODEC_ZSTD, clevel=args.clevel, shuffle=0)
    cap = comp.max_bytes(N_CHUNKS)
    frames = torch.empty(cap, dtype=torch.uint8, device=dev)
    off = torch.empty(N_CHUNKS + 1, dtype=torch.int64, device=dev)
    comp.run_ptr(src.data_ptr(), CHUNK, N_CHUNKS, frames.data_ptr(), cap, off.data_ptr(), stream)
    torch.cuda.synchronize()
    total = int(off[-1].item())
    out = torch.empty(layer_bytes, dtype=torch.uint8, device=dev)
    status = torch.empty(N_CHUNKS, dtype=torch.int32, device=dev)
    decs = {m: aqz.Decompressor(CHUNK, N_CHUNKS, codecs=mask[m]) for m in modes}
    row = {"tool": "tools/decode_rate.py --zstd-parallel " + args.zstd_parallel,
           "layer": "C2 level 0: 64 chunks of 256x256x64 u16", "layer_bytes": layer_bytes,
           "codec": "zstd", "clevel": args.clevel, "compressed_bytes": total,
           "ratio": round(layer_bytes / total, 3), "repetitions": args.repetitions,
           "timing": "one call per repetition, modes interleaved; decode: HIP events on the "
                     "stream; verify: host clock around verify_layer + verify_result"}

    def run(m):
        decs[m].run_ptr(frames.data_ptr(), cap, off.data_ptr(), N_CHUNKS, out.data_ptr(), CHUNK,
                        CHUNK, status.data_ptr(), stream)

    for m in modes:     # warm-up, and the bytes
        out.zero_()
        run(m)
        torch.cuda.synchronize()
        row[m + "_decode_exact"] = bool(torch.equal(out, src)) and not bool(status.any())
        row[m + "_scratch_bytes"] = decs[m].scratch_bytes()
        if m == "parallel":
            row["parallel_counts"] = decs[m].last_run_counts()
    ms = {m: [] for m in modes}
    for _ in range(args.repetitions):
        for m in modes:
            ms[m].append(event_ms(lambda: run(m)))
    for m in modes:
        row[m + "_decode_ms"] = [round(v, 3) for v in ms[m]]
        row[m + "_decode_gbs_slowest"] = gbs(max(ms[m]))
        row[m + "_decode_gbs_fastest"] = gbs(min(ms[m]))
    host = []
    if libzstd() is not None:
        o = off.cpu().numpy()
        k = min(args.host_chunks, N_CHUNKS)
        fr = [frames[int(o[i]):int(o[i + 1])].cpu().numpy().tobytes() for i in range(k)]
        zstd_decode(fr[0], CHUNK)
        for _ in range(args.repetitions):
            t0 = time.perf_counter()
            for f in fr:
                zstd_decode(f, CHUNK)
            host.append(k * CHUNK / (time.perf_counter() - t0) / 1e9)
        row["libzstd_1core_decode_gbs"] = [round(v, 2) for v in host]
        row["libzstd_chunks"] = k
    for d in decs.values():
        d.close()
    comp.close()
    del frames, out

    # the same layer through a stage per mode, verified against the resident chunks
    dims = [(aqz.TIME, 0, PLANES, 1), (aqz.SPACE, SIDE, 256, 1), (aqz.SPACE, SIDE, 256, 1)]
    stages = {}
    for m in modes:
        st = aqz.Stage(dims, aqz.UINT16, aqz.MEAN, multiscale=False, layer_slots=1,
                       max_batch_frames=PLANES)
        st.append_ptr(src.data_ptr(), PLANES, aqz.MEM_DEVICE)
        st.synchronize()
        st.verify_prepare(mask[m])
        st.compress_layer(0, 0, codec=aqz.CODEC_ZSTD, clevel=args.clevel, shuffle=0)
        st.compressed_offsets(0, 0)
        row[m + "_verify_result"] = list(st.verify_layer(0, 0))      # warm-up
        stages[m] = st
    vms = {m: [] for m in modes}
    for _ in range(args.repetitions):
        for m in modes:
            t0 = time.perf_counter()
            stages[m].verify_layer(0, 0)
            vms[m].append((time.perf_counter() - t0) * 1e3)
    for m in modes:
        row[m + "_verify_ms"] = [round(v, 3) for v in vms[m]]
        row[m + "_verify_gbs_slowest"] = gbs(max(vms[m]))
        row[m + "_verify_gbs_fastest"] = gbs(min(vms[m]))
        stages[m].close()
    if "parallel" in modes:
        slow = layer_bytes / max(ms["parallel"]) / 1e6
        cond = {}
        if "serial" in modes:
            cond["above_serial_fastest"] = bool(slow > layer_bytes / min(ms["serial"]) / 1e6)
        if host:
            cond["above_libzstd_1core_fastest"] = bool(slow > max(host))
        row["condition"] = cond
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-chunks", type=int, default=8)
    ap.add_argument("--out", default=None,
                    help="default profiles/r07_decode_rate.jsonl, with --zstd-parallel "
                         "profiles/r09_zstd_parallel_rate.jsonl")
    ap.add_argument("--codecs", default="lz4", help="comma list of lz4, blosc-zstd, zstd")
    ap.add_argument("--clevel", type=int, default=5)
    ap.add_argument("--zstd-parallel", choices=("off", "on", "both"), default="off",
                    help="the plain-zstd layer through AQZ_DECODE_ZSTD_PARALLEL (on), or "
                         "through both decoders, interleaved (both)")
    ap.add_argument("--repetitions", type=int, default=3,
                    help="--zstd-parallel: timed repetitions of each mode (at least 3)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "r07_decode_rate.jsonl" if
                                args.zstd_parallel == "off" else "r09_zstd_parallel_rate.jsonl")
    if args.zstd_parallel != "off":
        args.repetitions = max(3, args.repetitions)
        dev = torch.device("cuda", 0)
        row = zstd_parallel_row(args, dev, torch.cuda.current_stream().cuda_stream, camera(dev))
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(row) + "\n")
        return
    codec_ids = {"lz4": aqz.CODEC_BLOSC_LZ4, "blosc-zstd": aqz.CODEC_BLOSC_ZSTD,
                 "zstd": aqz.CODEC_ZSTD}
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    src = camera(dev)
    layer_bytes = N_CHUNKS * CHUNK
    gbs = lambda ms: round(layer_bytes / ms / 1e6, 1)
    try:
        from codec_helpers import libblosc, libblosc_decode
        have_blosc = libblosc() is not None
    except Exception:
        have_blosc = False
    rows = []
    cases = [(name, sh) for name in args.codecs.split(",")
             for sh in ((0,) if name == "zstd" else (1, 2))]
    for name, shuffle in cases:
        codec = codec_ids[name]
        zstd = name != "lz4"
        comp = aqz.Compressor(CHUNK, 2, codec=codec, clevel=args.clevel, shuffle=shuffle)
        cap = comp.max_bytes(N_CHUNKS)
        frames = torch.empty(cap, dtype=torch.uint8, device=dev)
        off = torch.empty(N_CHUNKS + 1, dtype=torch.int64, device=dev)
        c_ms = timed(lambda: comp.run_ptr(src.data_ptr(), CHUNK, N_CHUNKS, frames.data_ptr(), cap,
                                          off.data_ptr(), stream), args.reps)
        total = int(off[-1].item())
        dec = aqz.Decompressor(CHUNK, N_CHUNKS,
                               codecs=aqz.DECODE_CODEC_ZSTD if zstd else aqz.DECODE_CODEC_LZ4)
        out = torch.empty(layer_bytes, dtype=torch.uint8, device=dev)
        status = torch.empty(N_CHUNKS, dtype=torch.int32, device=dev)
        d_ms = timed(lambda: dec.run_ptr(frames.data_ptr(), cap, off.data_ptr(), N_CHUNKS,
                                         out.data_ptr(), CHUNK, CHUNK, status.data_ptr(), stream),
                     args.reps)
        exact = bool(torch.equal(out, src)) and not bool(status.any())
        row = {"tool": "tools/decode_rate.py", "layer": "C2 level 0: 64 chunks of 256x256x64 u16",
               "layer_bytes": layer_bytes, "codec": "blosc-" + name if name == "lz4" else name,
               "clevel": args.clevel, "shuffle": shuffle,
               "decoder_scratch_bytes": dec.scratch_bytes(),
               "blocksize": comp.blocksize, "compressed_bytes": total,
               "ratio": round(layer_bytes / total, 3), "reps": args.reps,
               "compress_ms": round(c_ms, 3), "compress_gbs": gbs(c_ms),
               "decode_ms": round(d_ms, 3), "decode_gbs": gbs(d_ms), "decode_exact": exact}
        if name == "zstd":
            from codec_helpers import libzstd, zstd_decode
            if libzstd() is not None:
                o = off.cpu().numpy()
                k = min(args.host_chunks, N_CHUNKS)
                host = [frames[int(o[i]):int(o[i + 1])].cpu().numpy().tobytes() for i in range(k)]
                zstd_decode(host[0], CHUNK)
                t0 = time.perf_counter()
                for fr in host:
                    zstd_decode(fr, CHUNK)
                dt = time.perf_counter() - t0
                row["libzstd_1core_decode_gbs"] = round(k * CHUNK / dt / 1e9, 2)
        elif have_blosc:
            o = off.cpu().numpy()
            k = min(args.host_chunks, N_CHUNKS)
            host = [frames[int(o[i]):int(o[i + 1])].cpu().numpy().tobytes() for i in range(k)]
            libblosc_decode(host[0])
            t0 = time.perf_counter()
            for fr in host:
                libblosc_decode(fr)
            dt = time.perf_counter() - t0
            row["cblosc_1core_decode_gbs"] = round(k * CHUNK / dt / 1e9, 2)
            row["cblosc_chunks"] = k
        dec.close()
        comp.close()
        del frames, out

        # the same layer through a stage: appended from the device, compressed
        # on the hand-off stream, then verified against the resident chunks
        dims = [(aqz.TIME, 0, PLANES, 1), (aqz.SPACE, SIDE, 256, 1),
                (aqz.SPACE, SIDE, 256, 1)]
        st = aqz.Stage(dims, aqz.UINT16, aqz.MEAN, multiscale=False, layer_slots=1,
                       max_batch_frames=PLANES)
        st.append_ptr(src.data_ptr(), PLANES, aqz.MEM_DEVICE)
        st.synchronize()
        if zstd:
            st.verify_prepare(aqz.DECODE_CODEC_ZSTD)
        st.compress_layer(0, 0, codec=codec, clevel=args.clevel, shuffle=shuffle)
        st.compressed_offsets(0, 0)
        res = st.verify_layer(0, 0)     # warm-up (allocates the decoder state)
        t0 = time.perf_counter()
        for _ in range(args.reps):
            res = st.verify_layer(0, 0)
        v_ms = (time.perf_counter() - t0) * 1e3 / args.reps
        row.update({"verify_ms": round(v_ms, 3), "verify_gbs": gbs(v_ms),
                    "verify_result": list(res),
                    "verify_timing": "host clock around verify_layer + verify_result"})
        st.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
