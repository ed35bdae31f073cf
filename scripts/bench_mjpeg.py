"""256 seeded smooth-plus-noise frames of 512 x 512 through the JPEG encoder (instag_amd/mjpeg.py) at quality 90,
4:2:0: ``encode`` alone (the bytes stay on the device) and ``encode_bytes`` (with the copy to the host), beside the
route without it on the same machine in the same session: the raw frames copied to the host and
``PIL.Image.save(quality=90)`` on one thread, on 16 threads (Pillow keeps the interpreter lock while it encodes into
memory, so these gain nothing) and in 16 processes that read the frames from shared memory and send the bytes back.

Medians of WINDOWS alternating windows of one pass over all frames, after a warm-up pass of each path; ``encode`` is
timed with device events, the three paths that end on the host with the wall clock around a synchronised window.  The
warm-up pass checks the device's bytes against the statement on the first frames.  No figure here is a pass condition.

    python scripts/bench_mjpeg.py --json profiles/mjpeg_bench.json
"""
import argparse, io, json, os, statistics, sys, time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from _bench_frames import operator_kernels, seeded_frames, window
from instag_amd import mjpeg as M

WINDOWS = 5
dev = torch.device("cuda")
_SHARED = {}


def _attach(name, shape):
    """A worker process's view of the frames in shared memory (it never touches the GPU)."""
    import numpy as np
    from multiprocessing import shared_memory
    _SHARED["block"] = shared_memory.SharedMemory(name=name)
    _SHARED["frames"] = np.ndarray(shape, dtype=np.uint8, buffer=_SHARED["block"].buf)


def _save(frame):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, "JPEG", quality=90)
    return buf.getvalue()


def _save_shared(i):
    return _save(_SHARED["frames"][i])


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    host = seeded_frames(a.frames, a.size)
    frames = host.to(dev)
    enc = M.JpegEncoder(a.size, a.size, dev, quality=90, subsampling="4:2:0", max_batch=a.batch)

    def encode():
        return [enc.encode(frames[i:i + a.batch]) for i in range(0, a.frames, a.batch)]

    def encode_bytes():
        return enc.encode_bytes(frames)

    def pil(threads):
        raw = frames.cpu().numpy()
        if threads == 1:
            return [_save(f) for f in raw]
        with ThreadPoolExecutor(threads) as ex:
            return list(ex.map(_save, raw))

    import multiprocessing as mp
    import numpy as np
    from multiprocessing import shared_memory
    block = shared_memory.SharedMemory(create=True, size=host.numel())
    shared = np.ndarray(tuple(host.shape), dtype=np.uint8, buffer=block.buf)
    pool = mp.get_context("spawn").Pool(a.threads, initializer=_attach, initargs=(block.name, tuple(host.shape)))

    def pil_processes():
        shared[...] = frames.cpu().numpy()
        return pool.map(_save_shared, range(a.frames), chunksize=max(1, a.frames // (4 * a.threads)))

    got = encode_bytes()
    assert got[:4] == M.jpeg_encode_torch(host[:4], 90, "4:2:0")              # faster and different is not faster
    encode(), pil(1), pil(a.threads)
    assert pil_processes() == pil(1)
    assert int(enc.overflow.sum()) == 0
    theirs = pil(1)
    t = {"encode": [], "encode_bytes": [], "pil_1_thread": [], f"pil_{a.threads}_threads": [], f"pil_{a.threads}_processes": []}
    for _ in range(WINDOWS):
        t["encode"].append(window(encode))
        t["encode_bytes"].append(wall(encode_bytes))
        t["pil_1_thread"].append(wall(lambda: pil(1)))
        t[f"pil_{a.threads}_threads"].append(wall(lambda: pil(a.threads)))
        t[f"pil_{a.threads}_processes"].append(wall(pil_processes))
    pool.close()
    pool.join()
    block.close()
    block.unlink()
    res = dict(frames=a.frames, size=a.size, quality=90, subsampling="4:2:0", batch=a.batch, host_cpus=os.cpu_count(),
               mean_jpeg_bytes=sum(map(len, got)) / a.frames, mean_pil_jpeg_bytes=sum(map(len, theirs)) / a.frames,
               raw_frame_bytes=a.size * a.size * 3, capacity=enc.capacity)
    for k, v in t.items():
        ms = statistics.median(v)
        res[f"{k}_ms"], res[f"{k}_min_ms"], res[f"{k}_frames_per_s"] = ms, min(v), a.frames / (ms * 1e-3)
        print(f"{k:16s}: {ms:8.1f} ms for {a.frames} frames (min {min(v):.1f}), {res[f'{k}_frames_per_s']:.0f} frames/s", flush=True)
    res["kernels_one_chunk"] = operator_kernels(lambda: enc.encode(frames[:a.batch]))
    for k, v in res["kernels_one_chunk"].items():
        print(f"  {k:40s} {v}")
    print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
