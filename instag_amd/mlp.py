"""Fused bias-free ReLU MLP operator (HIP, f32 MFMA) behind ``motion_net.MLP``.

Boundary: the reference's ``MLP.forward`` (scene/motion_net.py:167-173) applied to the per-Gaussian
feature matrix [N, dim_in].  C ABI: instag_mlp_forward / instag_mlp_backward /
instag_linear_weight_grad_batched (include/instag_hip.h).
"""
from __future__ import annotations

import torch

from . import _lib, deferred
from ._lib import check, ptr


# multiply-add work launched so far (2 flops per MAC), read by bench.py for the MFMA roofline of the MLP kernels
STATS = {"fwd_flops": 0, "bwd_flops": 0}
MAX_WGRAD_JOBS = 16           # per launch (include/instag_hip.h)


def supported(dim_in, dim_hidden, dim_out, num_layers) -> bool:
    return num_layers in (2, 3) and 1 <= dim_in <= 96 and 1 <= dim_hidden <= 64 and 1 <= dim_out <= 32


def sign_words(N, dev):
    """One ReLU sign word per lane and 32-row tile of a hidden layer, [ceil(N/32), 64] (include/instag_hip.h): what the
    backward kernels read in place of the activations."""
    return torch.empty((N + 31) // 32, 64, dtype=torch.int32, device=dev)


def _forward(L, x, w1, w2, w3, keep):
    """MLP(x) for contiguous fp32 x [N,K0] and weights [out,in] (w3 None: two layers) -> (y, a1, a2, s1, s2): the hidden
    activations and ReLU sign words that the gradients read, None without ``keep`` (a2, s2: and with two layers)."""
    N, K0 = x.shape
    H = w1.shape[0]
    NL = 2 if w3 is None else 3
    O = (w2 if NL == 2 else w3).shape[0]
    y = torch.empty(N, O, dtype=torch.float32, device=x.device)
    a1 = torch.empty(N, H, dtype=torch.float32, device=x.device) if keep else None
    a2 = torch.empty(N, H, dtype=torch.float32, device=x.device) if (keep and NL == 3) else None
    s1 = sign_words(N, x.device) if keep else None
    s2 = sign_words(N, x.device) if (keep and NL == 3) else None
    check(L.instag_mlp_forward(ptr(x), ptr(w1), ptr(w2), ptr(w3), ptr(y), ptr(a1), ptr(a2), ptr(s1), ptr(s2),
                               N, K0, H, O, NL, _lib.current_stream()), "mlp_forward")
    STATS["fwd_flops"] += 2 * N * (K0 * H + (H * H if NL == 3 else 0) + H * O)
    return y, a1, a2, s1, s2


def _wgrad_launches(jobs):
    """Indices of the jobs of each launch: equal N, at most MAX_WGRAD_JOBS, at most one with virtual input rows."""
    by_n = {}
    for i, (dz, _, _) in enumerate(jobs):
        by_n.setdefault(dz.shape[0], []).append(i)
    for group in by_n.values():
        cur = []
        for i in group:
            if len(cur) == MAX_WGRAD_JOBS or (jobs[i][2] is not None and any(jobs[j][2] is not None for j in cur)):
                yield cur
                cur = []
            cur.append(i)
        yield cur


def weight_grads(jobs):
    """dW = dz^T @ inp, [O,K] fp32, for every job (dz [N,O], inp [N,K], virt) of one device, in job order: one launch
    for all jobs of one N (see _wgrad_launches).  ``virt`` = (aud, eye_pre, enc_a, enc_e): the input rows were never
    stored, they are cat(inp, aud * enc_a, relu(eye_pre) * enc_e) (glue._GlueSigma) and the kernel assembles them
    while loading; None: inp holds the rows."""
    L = _lib.lib()
    dev = jobs[0][0].device
    dws = [None] * len(jobs)
    for chunk in _wgrad_launches(jobs):
        arr = (_lib.WgradJob * len(chunk))()
        total, glue = 0, None
        for slot, i in enumerate(chunk):
            dz, inp, virt = jobs[i]
            N, O, K = dz.shape[0], dz.shape[1], inp.shape[1]
            if virt is not None:
                glue = (slot, virt)
                K += virt[0].shape[1] + virt[1].shape[1]
            dws[i] = torch.empty(O, K, dtype=torch.float32, device=dev)
            arr[slot] = _lib.WgradJob(dz.data_ptr(), inp.data_ptr(), dws[i].data_ptr(), N, O, K)
            total += (L.instag_linear_weight_grad_workspace_bytes(N, O, K) + 255) // 256 * 256
        ws = torch.empty(total, dtype=torch.uint8, device=dev)
        if glue is None:
            check(L.instag_linear_weight_grad_batched(arr, len(chunk), ptr(ws), total, _lib.current_stream()),
                  "linear_weight_grad_batched")
        else:
            slot, (aud, eye_pre, enc_a, enc_e) = glue
            check(L.instag_linear_weight_grad_batched_glue(arr, len(chunk), slot, ptr(aud), ptr(eye_pre), ptr(enc_a),
                                                           ptr(enc_e), aud.shape[1], eye_pre.shape[1], ptr(ws), total,
                                                           _lib.current_stream()), "linear_weight_grad_batched_glue")
    return dws


def emit_weight_grads(jobs, weights, wanted):
    """The weight gradients of one autograd node, for its backward to return: jobs[i] = (dz, inp, virt) yields the
    gradient of weights[i] (None: a two-layer MLP has no third), wanted[i] = the weight's ``needs_input_grad``.  Only the
    optimizer reads them: inside a ``deferred_grads`` block (instag_amd/deferred.py) whose node's weights are all leaf
    parameters they are queued for the block's batched launch and autograd gets None; otherwise they are computed
    now, in one launch."""
    slots = [i for i, job in enumerate(jobs) if job is not None and wanted[i]]
    grads = [None] * len(weights)
    if deferred.active() and all(w is None or w.is_leaf for w in weights):
        for i in slots:
            dz, inp, virt = jobs[i]
            deferred.defer_weight_grad(dz, inp, weights[i], virt)
    elif slots:
        for i, dw in zip(slots, weight_grads([jobs[i] for i in slots])):
            grads[i] = dw
    return grads


class _FusedMLP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, w2, w3):
        x = x.contiguous().float()
        w1c, w2c = w1.contiguous().float(), w2.contiguous().float()
        w3c = None if w3 is None else w3.contiguous().float()
        y, a1, a2, s1, s2 = _forward(_lib.lib(), x, w1c, w2c, w3c, any(ctx.needs_input_grad))
        ctx.save_for_backward(x, w1c, w2c, w3c, a1, a2, s1, s2)
        ctx.weights = (w1, w2, w3)          # the caller's tensors (leaf parameters in the deferred-gradient mode)
        return y

    @staticmethod
    def backward(ctx, dy):
        return mlp_backward(ctx.saved_tensors, dy, ctx.needs_input_grad[0], ctx.weights, ctx.needs_input_grad[1:])


def mlp_backward(saved, dy, want_dx, weights, wanted):
    """Backward launch of one MLP for what its forward saved -> (dx or None, dw1, dw2, dw3); see emit_weight_grads for
    ``weights`` and ``wanted``.  Shared by _FusedMLP and instag_amd/encode_mlp.py."""
    L = _lib.lib()
    x, w1, w2, w3, a1, a2, s1, s2 = saved
    (N, K0), H = x.shape, w1.shape[0]
    NL = 2 if w3 is None else 3
    O = dy.shape[1]
    dy = dy.contiguous().float()
    dev = dy.device
    dz1 = torch.empty(N, H, dtype=torch.float32, device=dev)
    dz2 = torch.empty(N, H, dtype=torch.float32, device=dev) if NL == 3 else None
    dx = torch.empty(N, K0, dtype=torch.float32, device=dev) if want_dx else None
    check(L.instag_mlp_backward(ptr(dy), ptr(s1), ptr(s2), ptr(w1), ptr(w2), ptr(w3), ptr(dz1), ptr(dz2), ptr(dx),
                                N, K0, H, O, NL, _lib.current_stream()), "mlp_backward")
    STATS["bwd_flops"] += 2 * N * (H * O + (H * H if NL == 3 else 0) + (K0 * H if dx is not None else 0))
    jobs = [(dz1, x, None)] + ([(dz2, a1, None), (dy, a2, None)] if NL == 3 else [(dy, a1, None), None])
    return (dx, *emit_weight_grads(jobs, weights, wanted))


class _SharedInputMLPs(torch.autograd.Function):
    """Two 2-layer MLPs over the SAME input x plus x itself as a third output (for the input's other consumers):
    (MLP_a(x), MLP_b(x), x).  The reference runs aud_ch_att_net(enc_x), eye_att_net(enc_x) and then concatenates
    enc_x into sigma_net's input (scene/motion_net.py:281-306), so autograd sums three gradients of enc_x with two
    elementwise launches; here the sum happens inside the backward kernel (instag_mlp2_backward; a shape pair without
    one runs the heads one by one, instag_mlp_backward_add)."""

    @staticmethod
    def forward(ctx, x, wa1, wa2, wb1, wb2):
        L = _lib.lib()
        x = x.contiguous().float()
        N, K0 = x.shape
        ws = [w.contiguous().float() for w in (wa1, wa2, wb1, wb2)]
        (HA, OA), (HB, OB) = (ws[0].shape[0], ws[1].shape[0]), (ws[2].shape[0], ws[3].shape[0])
        keep = any(ctx.needs_input_grad)          # forward only (inference, the jaw feature): nothing is kept
        ctx.weights = (wa1, wa2, wb1, wb2)
        ctx.fused = bool(L.instag_mlp2_supported(K0, HA, OA, HB, OB))
        if ctx.fused:
            # both heads in one launch: the tile of x is loaded once (csrc/mlp.hip: mlp2_forward_kernel)
            ya = torch.empty(N, OA, dtype=torch.float32, device=x.device)
            yb = torch.empty(N, OB, dtype=torch.float32, device=x.device)
            a1a = torch.empty(N, HA, dtype=torch.float32, device=x.device) if keep else None
            a1b = torch.empty(N, HB, dtype=torch.float32, device=x.device) if keep else None
            s1a = s1b = sign_words(N, x.device) if keep else None   # both heads' bits: A low half, B high half
            check(L.instag_mlp2_forward(ptr(x), ptr(ws[0]), ptr(ws[1]), ptr(ws[2]), ptr(ws[3]), ptr(ya), ptr(yb),
                                        ptr(a1a), ptr(a1b), ptr(s1a), N, K0, HA, OA, HB, OB, _lib.current_stream()),
                  "mlp2_forward")
            STATS["fwd_flops"] += 2 * N * (K0 * HA + HA * OA + K0 * HB + HB * OB)
        else:
            ya, a1a, _, s1a, _ = _forward(L, x, ws[0], ws[1], None, keep)
            yb, a1b, _, s1b, _ = _forward(L, x, ws[2], ws[3], None, keep)
        ctx.save_for_backward(x, ws[0], ws[1], a1a, s1a, ws[2], ws[3], a1b, s1b)
        return ya, yb, x.view_as(x)

    @staticmethod
    def backward(ctx, dya, dyb, dx_other):
        # (all three are tensors: autograd hands in zeros for an output that nothing read)
        return shared_input_backward(ctx.saved_tensors, ctx.fused, dya, dyb, dx_other, ctx.needs_input_grad[0],
                                     ctx.weights, ctx.needs_input_grad[1:])


def shared_input_backward(saved, fused, dya, dyb, dx_other, want_dx, weights, wanted):
    """Backward launch(es) of two MLPs over one input for what their forward saved -> (dx or None, four weight gradients);
    dx includes ``dx_other``, the gradient of the input's other consumers.  Shared by _SharedInputMLPs and
    instag_amd/encode_mlp.py."""
    L = _lib.lib()
    x, wa1, wa2, a1a, s1a, wb1, wb2, a1b, s1b = saved
    N, K0 = x.shape
    (HA, OA), (HB, OB) = (wa1.shape[0], wa2.shape[0]), (wb1.shape[0], wb2.shape[0])
    dev = x.device
    stream = _lib.current_stream()
    dx = torch.empty(N, K0, dtype=torch.float32, device=dev) if want_dx else None
    add = dx_other.contiguous().float() if want_dx else None
    dya, dyb = dya.contiguous().float(), dyb.contiguous().float()
    dz1a = torch.empty(N, HA, dtype=torch.float32, device=dev)
    dz1b = torch.empty(N, HB, dtype=torch.float32, device=dev)
    if fused:
        check(L.instag_mlp2_backward(ptr(dya), ptr(dyb), ptr(s1a), ptr(s1b), ptr(wa1), ptr(wa2), ptr(wb1),
                                     ptr(wb2), ptr(dz1a), ptr(dz1b), ptr(dx), ptr(add), N, K0, HA, OA, HB, OB,
                                     stream), "mlp2_backward")
    else:
        for dy, s1, w1, w2, dz1 in ((dya, s1a, wa1, wa2, dz1a), (dyb, s1b, wb1, wb2, dz1b)):
            check(L.instag_mlp_backward_add(ptr(dy), ptr(s1), None, ptr(w1), ptr(w2), None, ptr(dz1), None, ptr(dx),
                                            ptr(add), N, K0, w1.shape[0], w2.shape[0], 2, stream), "mlp_backward")
            add = dx                          # the second kernel adds onto what the first wrote
    STATS["bwd_flops"] += 2 * N * (HA * OA + HB * OB + (K0 * (HA + HB) if want_dx else 0))
    jobs = [(dz1a, x, None), (dya, a1a, None), (dz1b, x, None), (dyb, a1b, None)]
    return (dx, *emit_weight_grads(jobs, weights, wanted))


def shared_input_mlps(x, weights_a, weights_b):
    """(MLP_a(x), MLP_b(x), x_for_other_consumers) for two 2-layer bias-free ReLU MLPs: see _SharedInputMLPs."""
    return _SharedInputMLPs.apply(x, weights_a[0], weights_a[1], weights_b[0], weights_b[1])


def fused_mlp(x, weights):
    """x [N, K0] on the GPU; weights = list of 2 or 3 torch.nn.Linear weights ([out, in])."""
    w3 = weights[2] if len(weights) == 3 else None
    return _FusedMLP.apply(x, weights[0], weights[1], w3)
