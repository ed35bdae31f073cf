"""256 smooth-plus-noise frames of 512 x 512 as JPEG files (quality 90, 4:2:0), written once by PIL and once by this
project's ``JpegEncoder``, through the JPEG decoder (instag_amd/jpeg_decode.py): ``decode`` from the files' bytes (parse
and pack on the host, upload of the bytes, the kernels), beside the route without it on the same machine in the same
session: ``PIL.Image.open(...).convert("RGB")`` on one thread and the upload of the pixels.  Then the stages alone on
scans that are on the device already (``decode_into``, ``coefficients_of``, ``pixels``), the host's share (parse and
pack), and ``decode_into`` per ``sub_bits``.

Medians of WINDOWS alternating windows of one pass over all frames, after a warm-up pass of each path, timed with device
events around the window (they span the host's work inside it).  The warm-up pass checks the device's pixels against
PIL's on every frame.  No figure here is a pass condition.

    python scripts/bench_jpeg_decode.py --json profiles/jpeg_decode_bench.json
"""
import argparse, io, json, os, statistics, sys, time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from _bench_frames import operator_kernels, window
from instag_amd import jpeg_decode as D, mjpeg as M

WINDOWS = 5
SUB_BITS = (64, 256, 512, 1024, 2048, 4096)
dev = torch.device("cuda")


def typical_frames(n, size):
    """Smooth waves with a little noise, frame by frame another phase and seed."""
    y, x = np.mgrid[0:size, 0:size].astype(np.float64)
    out = np.empty((n, size, size, 3), np.uint8)
    for i in range(n):
        a = np.stack([128 + 110 * np.sin(x / 5.0 + y / 11.0 + 1 + 0.1 * i), 128 + 100 * np.cos(x / 7.0 - y / 3.0),
                      128 + 90 * np.sin(y / 4.0 + 0.3) * np.cos(x / 9.0 + 0.05 * i)], -1)
        a = a * 0.7 + 38 + np.random.default_rng(i).uniform(-6, 6, a.shape)
        out[i] = np.clip(np.rint(a), 0, 255)
    return torch.from_numpy(out)


def pil_write(frame):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, "JPEG", quality=90)
    return buf.getvalue()


def pil_read(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    host = typical_frames(a.frames, a.size)
    enc = M.JpegEncoder(a.size, a.size, dev, quality=90, subsampling="4:2:0")
    sources = {"pil": [pil_write(f) for f in host.numpy()], "encoder": enc.encode_bytes(host.to(dev))}
    chunks = lambda files: [files[i:i + a.batch] for i in range(0, a.frames, a.batch)]
    res = dict(frames=a.frames, size=a.size, quality=90, subsampling="4:2:0", batch=a.batch, host_cpus=os.cpu_count(),
               raw_frame_bytes=a.size * a.size * 3, default_sub_bits=D.SUB_BITS)
    for name, files in sources.items():
        dec = D.JpegDecoder(dev, max_batch=a.batch)
        infos = [D.parse_jpeg(f) for f in files]
        cap = max(i.scan[1] for i in infos)
        packed = [tuple(t.to(dev) for t in dec.pack(c, ci, capacity=cap)) for c, ci in zip(chunks(files), chunks(infos))]
        frames = torch.empty(a.batch, a.size, a.size, 3, dtype=torch.uint8, device=dev)
        status = torch.empty(a.batch, dtype=torch.int32, device=dev)
        coef = torch.empty(a.batch, M.block_count(a.size, a.size), 64, dtype=torch.int16, device=dev)
        quant = packed[0][3]

        def decode(d=dec):
            return [d.decode(c) for c in chunks(files)]

        def pil_upload():
            return [torch.from_numpy(np.stack([pil_read(f) for f in c])).to(dev) for c in chunks(files)]

        def stages(d=dec):
            for p in packed:
                d.decode_into(*p, "4:2:0", frames[:p[0].shape[0]], status[:p[0].shape[0]])

        def huffman(d=dec):
            for p in packed:
                d.coefficients_of(p[0], p[1], p[2], a.size, a.size, "4:2:0", coef=coef[:p[0].shape[0]], status=status[:p[0].shape[0]])

        def pixels(d=dec):
            for p in packed:
                d.pixels(coef[:p[0].shape[0]], p[3], a.size, a.size, "4:2:0", frames=frames[:p[0].shape[0]])

        def host_side(d=dec):
            for c in chunks(files):
                d.pack(c, [D.parse_jpeg(f) for f in c])

        # faster and different is not faster: every frame equals PIL's (this pass is also the warm-up)
        got, want = decode(), pil_upload()
        assert all(int(s.abs().sum()) == 0 for _, s in got)
        assert all(torch.equal(g, w) for (g, _), w in zip(got, want))
        stages(), huffman(), pixels()
        t = {"decode": [], "pil_decode_and_upload": [], "kernels_all_stages": [], "kernels_unstuff_huffman": [],
             "kernels_idct_colour": [], "host_parse_and_pack": []}
        for _ in range(WINDOWS):
            t["decode"].append(window(decode))
            t["pil_decode_and_upload"].append(window(pil_upload))
            t["kernels_all_stages"].append(window(stages))
            t["kernels_unstuff_huffman"].append(window(huffman))
            t["kernels_idct_colour"].append(window(pixels))
            t["host_parse_and_pack"].append(wall(host_side))
        r = dict(mean_file_bytes=sum(map(len, files)) / a.frames, mean_scan_bytes=sum(i.scan[1] for i in infos) / a.frames,
                 capacity=cap)
        print(f"[{name}] {r['mean_file_bytes']:.0f} bytes per file", flush=True)
        for k, v in t.items():
            ms = statistics.median(v)
            r[f"{k}_ms"], r[f"{k}_min_ms"], r[f"{k}_frames_per_s"] = ms, min(v), a.frames / (ms * 1e-3)
            print(f"  {k:26s}: {ms:8.1f} ms for {a.frames} frames (min {min(v):.1f}), {r[f'{k}_frames_per_s']:.0f} frames/s", flush=True)
        table = {}
        decs = {sb: D.JpegDecoder(dev, max_batch=a.batch, sub_bits=sb) for sb in SUB_BITS}
        for sb, d in decs.items():
            stages(d)
            torch.cuda.synchronize()
            assert int(status.abs().sum()) == 0 and torch.equal(frames[:want[-1].shape[0]], want[-1])
            table[sb] = []
        for _ in range(WINDOWS):
            for sb, d in decs.items():
                table[sb].append(window(lambda: stages(d)))
        r["sub_bits_ms"] = {str(sb): statistics.median(v) for sb, v in table.items()}
        for sb, v in table.items():
            print(f"  sub_bits {sb:5d}: {statistics.median(v):8.2f} ms for {a.frames} frames (min {min(v):.2f})", flush=True)
        r["kernels_one_chunk"] = operator_kernels(lambda: dec.decode_into(*packed[0], "4:2:0", frames, status))
        for k, v in r["kernels_one_chunk"].items():
            print(f"  {k:40s} {v}")
        res[name] = r
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
