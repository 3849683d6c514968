#!/usr/bin/env python3
"""What a PNG frame costs up to its pixels being in device memory: the device decoder against
Pillow on this machine's CPU plus the upload, for the bench clip's rendered frame and for seeded noise, at 4K and 1080p,
the files written by PngEncoder(index=True) at the default band.

  host     (a) Pillow's decode of the file to an RGB array (one CPU thread) and the upload of that array: the path a
           frame took before the device decoder.
  device   (b) PngDecoder.decode of the same file (the walk, the file's upload, the kernels, the status and the rows'
           sums coming down): host clock around call and wait; and the kernels apart, from the library's own event
           profiler in a pass of its own.
  plans    the unfilter kernel alone (event profiler) on a zlib-built file of the rendered frame with every row Paeth --
           one segment, one wave: its worst plan -- and with every row None -- a segment a row: its best.
  check    the device's pixels are Pillow's, bit for bit.

    python tools/bench_pngdec.py [--out profiles/pngdec_bench.json] [--csv profiles/pngdec_kernel_stats.csv]

Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import struct
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SIZES = {"4k": (2160, 3840), "1080p": (1080, 1920)}
KERNELS = ("pd_crc", "pd_inflate", "pd_rows", "pd_unfilter")


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def forced_file(image, filter_type, band_rows):
    """An indexed file of `image` with every row of one filter type (0 None or 4 Paeth), its bands zlib level 1 with a
    full flush each (tests/pngdec_ref.build's format, without its five candidates in memory)."""
    h, w, _ = image.shape
    cur = image.reshape(h, 3 * w).astype(np.int16)
    if filter_type == 4:
        a = np.zeros_like(cur)
        a[:, 3:] = cur[:, :-3]
        b = np.zeros_like(cur)
        b[1:] = cur[:-1]
        c = np.zeros_like(cur)
        c[:, 3:] = b[:, :-3]
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        cur = cur - np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    rows = np.empty((h, 1 + 3 * w), np.uint8)
    rows[:, 0] = filter_type
    rows[:, 1:] = cur.astype(np.uint8)
    n_bands = -(-h // band_rows)
    co = zlib.compressobj(1, zlib.DEFLATED, -15)
    out = [b"\x89PNG\r\n\x1a\n", chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)),
           chunk(b"tfBX", struct.pack(">BBHII", 1, 0, 0, band_rows, n_bands)), chunk(b"IDAT", b"\x78\x01")]
    for band in range(n_bands):
        out.append(chunk(b"IDAT", co.compress(rows[band * band_rows:(band + 1) * band_rows].tobytes()) + co.flush(zlib.Z_FULL_FLUSH)))
    out.append(chunk(b"IDAT", co.flush(zlib.Z_FINISH) + struct.pack(">I", zlib.adler32(rows.tobytes()))))
    out.append(chunk(b"IEND", b""))
    return b"".join(out)


def device_runs(dec, data, reps):
    """(host-clock milliseconds per decode, {kernel: (launches, ms per launch)})."""
    from bench_jpeg import spread
    from transflow_amd import _lib
    from transflow_amd.device import sync
    from transflow_amd.pngdec import probe
    info = probe(data)
    dec.decode(data, info=info).close()
    whole = []
    for _ in range(reps):
        t0 = time.perf_counter()
        pix = dec.decode(data, info=info)
        sync()
        whole.append((time.perf_counter() - t0) * 1e3)
        pix.close()
    _lib.profile(True, "pd_")
    for _ in range(reps):
        dec.decode(data, info=info).close()
    sync()
    report = _lib.profile_report()
    _lib.profile(False)
    kernels = {k: {"launches": report[k][0], "ms_per_launch": report[k][1] / report[k][0]} for k in KERNELS if k in report}
    return spread(whole), kernels


def measure(image, h, w, reps, host_reps):
    from bench_jpeg import spread
    from transflow_amd.device import DevBuffer, sync
    from transflow_amd.png import PngEncoder
    from transflow_amd.pngdec import PngDecoder, pillow_decode, probe
    enc = PngEncoder(h, w, index=True)
    data = enc.encode(image)
    band_rows = enc.band_rows
    enc.close()
    info = probe(data)
    dec = PngDecoder(w, h, max_file_bytes=h * w * 4 + 65536)
    pix = dec.decode(data, info=info)
    want = pillow_decode(data)
    same = bool(np.array_equal(np.asarray(pix), want))
    pix.close()
    whole, kernels = device_runs(dec, data, reps)
    decode_ms, upload_ms = [], []
    dev = DevBuffer(h * w * 3)
    for _ in range(host_reps):
        t0 = time.perf_counter()
        array = pillow_decode(data)
        t1 = time.perf_counter()
        dev.upload(array)
        sync()
        t2 = time.perf_counter()
        decode_ms.append((t1 - t0) * 1e3), upload_ms.append((t2 - t1) * 1e3)
    dev.close()
    types = np.bincount([int(t) for t in _filter_types(data, info)], minlength=5).tolist()
    out = {"file_bytes": len(data), "band_rows": band_rows, "bands": info.n_bands, "rows_of_each_filter_type": types,
           "device_per_frame_ms": whole, "kernels": kernels, "kernels_ms": sum(v["ms_per_launch"] for v in kernels.values()),
           "pillow_decode_ms": spread(decode_ms), "upload_raw_ms": spread(upload_ms), "pixels_are_pillows": same}
    out["host_per_frame_ms"] = out["pillow_decode_ms"]["median_ms"] + out["upload_raw_ms"]["median_ms"]
    out["host_over_device"] = out["host_per_frame_ms"] / whole["median_ms"]
    dec.close()
    return out, None


def _filter_types(data, info):
    """The rows' filter types: the bands are blocks of one deflate stream."""
    d = zlib.decompressobj(-15)
    stream = b"".join(d.decompress(data[off:off + n]) for off, n in info.bands)
    return np.frombuffer(stream, np.uint8).reshape(info.height, 1 + 3 * info.width)[:, 0]


def plans(image, h, w, band_rows, reps):
    """The unfilter kernel on the all-Paeth and the all-None file of the same image."""
    from transflow_amd.pngdec import PngDecoder, pillow_decode
    out = {}
    dec = PngDecoder(w, h, max_file_bytes=h * w * 4 + 65536)
    for name, filter_type in (("all_paeth", 4), ("all_none", 0)):
        data = forced_file(image, filter_type, band_rows)
        pix = dec.decode(data)
        same = bool(np.array_equal(np.asarray(pix), image))
        pix.close()
        whole, kernels = device_runs(dec, data, reps)
        out[name] = {"file_bytes": len(data), "device_per_frame_ms": whole, "kernels": kernels, "pixels_are_the_image": same,
                     "unfilter_ms": kernels.get("pd_unfilter", {}).get("ms_per_launch")}
    dec.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--csv")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--sizes", default="4k,1080p")
    args = ap.parse_args()
    import bench
    from bench_jpeg import rendered_frame
    from tests import png_ref
    result = {"tool": "bench_pngdec", "host": bench.host_description(), "sizes": {}}
    csv = []
    for name in args.sizes.split(","):
        h, w = SIZES[name]
        comp, layer = rendered_frame(h, w)
        frame = np.array(comp.download())
        del comp, layer
        entry = {"height": h, "width": w}
        for label, image in (("rendered", frame), ("noise", png_ref.noise_image(h, w, 11))):
            entry[label], _ = measure(image, h, w, args.reps, args.host_reps)
            for k, v in entry[label]["kernels"].items():
                csv.append((name, label, k, v["launches"], v["ms_per_launch"]))
        entry["unfilter_plans"] = plans(frame, h, w, entry["rendered"]["band_rows"], max(3, args.reps // 2))
        for label, run in entry["unfilter_plans"].items():
            for k, v in run["kernels"].items():
                csv.append((name, label, k, v["launches"], v["ms_per_launch"]))
        result["sizes"][name] = entry
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if args.csv:
        with open(args.csv, "w") as f:
            f.write("size,file,kernel,launches,ms_per_launch\n")
            for row in csv:
                f.write("%s,%s,%s,%d,%.6f\n" % row)


if __name__ == "__main__":
    main()
