"""Inputs, references and a guarded ctypes caller for the tests of the batched weight-gradient launch
(csrc/mlp.hip: weight_grad_batched_kernel + weight_grad_reduce_batched_kernel; include/instag_hip.h:
instag_linear_weight_grad, instag_linear_weight_grad_batched, instag_linear_weight_grad_batched_glue).

Two kinds of data.  int_inputs: small non-zero integers, for which every fp32 partial sum is an integer below 2^24, so
every summation order is exact and the kernel must equal the fp64 reference bit for bit.  float_inputs: clamped normals,
checked element by element against rounding_bound, the standard gamma_D bound of a sum whose terms pass through at most D
fp32 roundings (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 4.2), with D counted from the
kernel's documented partition of the rows.  Importing this module needs no GPU."""
import collections
import ctypes as C
import math

import torch

CANARY = 256                       # bytes of known content before and after every dw and behind the workspace
U = 2.0 ** -24                     # unit roundoff of fp32


def reference(dz, inp):
    """dW = dz^T @ inp in fp64 on the CPU."""
    return dz.detach().cpu().double().t() @ inp.detach().cpu().double()


def virtual_rows(inp, aud, eye_pre, enc_a, enc_e):
    """The fp32 rows cat(inp, aud * enc_a, relu(eye_pre) * enc_e) that the glue entry point assembles while loading:
    each product is rounded once in fp32, here as in the kernel, so the operands are the same bit for bit."""
    inp, aud, eye_pre, enc_a, enc_e = (t.detach().cpu().float() for t in (inp, aud, eye_pre, enc_a, enc_e))
    return torch.cat([inp, aud * enc_a, torch.relu(eye_pre) * enc_e], dim=1).contiguous()


def _generator(N, width, seed):
    return torch.Generator().manual_seed(1000003 * int(seed) + 977 * int(N) + int(width))


def int_inputs(N, width, seed):
    """[N,width] fp32 (width None: [N]) of integers drawn from {-3,..,-1,1,..,3}: no zeros, both signs.  A product of
    three such values is at most 27, so sums over N <= 600 000 rows stay below 2^24 and are exact in fp32."""
    shape = (N,) if width is None else (N, width)
    g = _generator(N, width or 0, seed)
    mag = torch.randint(1, 4, shape, generator=g)
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mag * sign).float()


def float_inputs(N, width, seed):
    """[N,width] fp32 (width None: [N]) seeded normals with |x| clamped to [1e-3, 8]: no product of two or three of
    them is subnormal."""
    shape = (N,) if width is None else (N, width)
    x = torch.randn(shape, generator=_generator(N, width or 0, seed))
    sign = torch.where(x < 0, -1.0, 1.0)
    return (sign * x.abs().clamp(1e-3, 8.0)).float()


def partials(L, N, O, K):
    """Number of per-workgroup partial matrices the launch sums, from the public ABI."""
    return L.instag_linear_weight_grad_workspace_bytes(N, O, K) // (4 * O * K)


def rounding_bound(dz, inp, partials):
    """Per-element bound of |fp32 dW - fp64 dW|: gamma_D * (|dz|^T |inp|), gamma_D = D u / (1 - D u), u = 2^-24.
    D counts the roundings one term passes through: 1 for the unfused product, one per row of the longest chain
    (a workgroup's ceil(N / partials) rows, rounded up to even: + 1), at most 3 in the LDS combine of the row splits,
    ceil(partials / 4) in the reduce kernel's per-group sums and 3 in its final sum; 8 covers the fixed terms.  Holds
    for any order of those sums."""
    N = dz.shape[0]
    D = math.ceil(N / partials) + 1 + math.ceil(partials / 4) + 8
    gamma = D * U / (1.0 - D * U)
    return gamma * (dz.detach().cpu().double().abs().t() @ inp.detach().cpu().double().abs())


def guarded(t, rows=64):
    """t's values as a contiguous view into one larger allocation with ``rows`` rows of NaN in front and behind: a read
    outside the job's rows that reaches a sum shows as NaN in the result, and cannot fault."""
    buf = torch.full((t.shape[0] + 2 * rows, *t.shape[1:]), float("nan"), dtype=t.dtype, device=t.device)
    view = buf[rows:rows + t.shape[0]]
    view.copy_(t)
    assert view.is_contiguous()
    return view


def _canary(device):
    return ((torch.arange(CANARY, dtype=torch.int32) * 37 + 11) % 251).to(torch.uint8).to(device)


Run = collections.namedtuple("Run", "dws rc intact error")


def _job(job):
    """(dz, inp) or a dict with dz, inp (None: NULL) and optional N, O, K (default: from the tensors' shapes) and
    dw=False (NULL) -> (dz, inp, N, O, K, wants_dw)"""
    if not isinstance(job, dict):
        job = {"dz": job[0], "inp": job[1]}
    dz, inp = job.get("dz"), job.get("inp")
    N = job["N"] if "N" in job else dz.shape[0]
    O = job["O"] if "O" in job else dz.shape[1]
    K = job["K"] if "K" in job else inp.shape[1]
    return dz, inp, N, O, K, job.get("dw", True)


def _addr(t):
    return None if t is None else t.data_ptr()


class _Outputs:
    """dw buffers filled with 0xFF bytes (NaN) between two canaries, and a workspace of ``nbytes`` 0xFF bytes with a
    canary directly behind its last byte."""

    def __init__(self, counts, nbytes, device):
        self.canary = _canary(device)
        self.bufs = []
        for count in counts:
            buf = torch.full((2 * CANARY + 4 * count,), 0xFF, dtype=torch.uint8, device=device)
            buf[:CANARY] = self.canary
            buf[CANARY + 4 * count:] = self.canary
            self.bufs.append(buf)
        self.counts = counts
        self.nbytes = nbytes
        self.ws = torch.full((nbytes + CANARY,), 0xFF, dtype=torch.uint8, device=device)
        self.ws[nbytes:] = self.canary
        assert self.ws.data_ptr() % 256 == 0

    def dw_ptr(self, i):
        return self.bufs[i].data_ptr() + CANARY

    def dw(self, i, O, K):
        return self.bufs[i][CANARY:CANARY + 4 * self.counts[i]].view(torch.float32).view(O, K)

    def intact(self):
        ok = torch.equal(self.ws[self.nbytes:], self.canary)
        for buf, count in zip(self.bufs, self.counts):
            ok = ok and torch.equal(buf[:CANARY], self.canary) and torch.equal(buf[CANARY + 4 * count:], self.canary)
        return ok


def layout(L, dims):
    """Workspace layout of include/instag_hip.h for jobs of (N, O, K): every job's partials start on a 256-byte
    boundary, the last job's bytes are not rounded up -> (offsets, total bytes)."""
    offsets, off, end = [], 0, 0
    for N, O, K in dims:
        offsets.append(off)
        end = off + L.instag_linear_weight_grad_workspace_bytes(N, O, K)
        off = (end + 255) // 256 * 256
    return offsets, end


def run_jobs(jobs, glue=None, workspace_bytes=None):
    """One call of instag_linear_weight_grad_batched, or of instag_linear_weight_grad_batched_glue with
    glue = (slot, aud, eye_pre, enc_a, enc_e) (the job in ``slot`` then has K = inp.shape[1] + KA + KE), on device
    tensors.  ``workspace_bytes``: the size told to the library instead of the documented one (the allocation stays).
    -> Run(dws, return code, every canary intact, instag_last_error())"""
    from instag_amd import _lib
    L = _lib.lib()
    parsed = [_job(j) for j in jobs]
    if glue is not None:
        slot, aud, eye_pre, enc_a, enc_e = glue
        if 0 <= slot < len(parsed) and not (isinstance(jobs[slot], dict) and "K" in jobs[slot]):
            dz, inp, N, O, K, want = parsed[slot]
            parsed[slot] = (dz, inp, N, O, K + enc_a.numel() + enc_e.numel(), want)
    ok_dims = [(N, O, K) for _, _, N, O, K, _ in parsed if N >= 1 and 1 <= O <= 64 and 1 <= K <= 96]
    total = layout(L, ok_dims)[1] if len(ok_dims) == len(parsed) else 1 << 20
    out = _Outputs([max(1, O * K) for _, _, _, O, K, _ in parsed], total, "cuda")
    arr = (_lib.WgradJob * len(parsed))()
    for i, (dz, inp, N, O, K, want) in enumerate(parsed):
        arr[i] = _lib.WgradJob(_addr(dz), _addr(inp), out.dw_ptr(i) if want else None, N, O, K)
    nbytes = total if workspace_bytes is None else workspace_bytes
    stream = _lib.current_stream()
    if glue is None:
        rc = L.instag_linear_weight_grad_batched(arr, len(parsed), C.c_void_p(out.ws.data_ptr()), nbytes, stream)
    else:
        rc = L.instag_linear_weight_grad_batched_glue(arr, len(parsed), slot, _lib.ptr(aud), _lib.ptr(eye_pre),
                                                      _lib.ptr(enc_a), _lib.ptr(enc_e), enc_a.numel(), enc_e.numel(),
                                                      C.c_void_p(out.ws.data_ptr()), nbytes, stream)
    error = L.instag_last_error() if rc != 0 else b""
    torch.cuda.synchronize()
    dws = [out.dw(i, O, K) if O * K >= 1 else None for i, (_, _, _, O, K, _) in enumerate(parsed)]
    return Run(dws, rc, out.intact(), error)


def run_single(dz, inp, workspace_bytes=None):
    """instag_linear_weight_grad for one job, behind the same prefill and canaries as run_jobs."""
    from instag_amd import _lib
    L = _lib.lib()
    (N, O), K = dz.shape, inp.shape[1]
    total = L.instag_linear_weight_grad_workspace_bytes(N, O, K)
    out = _Outputs([O * K], total, "cuda")
    rc = L.instag_linear_weight_grad(_lib.ptr(dz), _lib.ptr(inp), C.c_void_p(out.dw_ptr(0)),
                                     C.c_void_p(out.ws.data_ptr()), total if workspace_bytes is None else workspace_bytes,
                                     N, O, K, _lib.current_stream())
    error = L.instag_last_error() if rc != 0 else b""
    torch.cuda.synchronize()
    return Run([out.dw(0, O, K)], rc, out.intact(), error)
