"""Inputs, statements and bars of the fused loss kernels' tests (csrc/ssim.hip: l1_ssim_*, face_loss_* in the face, mouth
and plain modes; tests/test_loss_kernels_gpu.py on the device, tests/test_loss_helpers_host.py for the conditions on the
inputs).

Inputs.  ``pair(kind, C, H, W, seed)`` makes two float32 images in [0, 1] on the fly:
  noise      x uniform, y = clamp(x + 0.2 randn): large windowed variances, nothing cancels -- the control, whose bars are
             tight enough that one pixel counted twice or left out cannot pass;
  smooth     a shading with periods of 50 to 150 px, x with 0.01 randn on top, y with a 0.03 ripple (31 / 47 px): windowed
             variances of the size of C2 = 9e-4, texture right up to every border;
  composite  the smooth pair inside a disc (r < 0.30 of the frame), the constant background BG outside it in three
             zones: 0.30 <= r < 0.40 where x is up to 0.02 off the background (the alpha bleed of a render) and y is the
             background, r >= 0.40 where x == y == background exactly, and the bottom (H + 1) // 6 rows where x and y are
             both saturated to exactly 0 or 1 (a square wave, shifted between the two).  1x1 keeps the disc only; 5x7 keeps
             all zones, its x == y zone and its strip below 16 pixels; from 11x11 on both hold at least 16;
  dark       the smooth pair times 0.029: mu1^2 + mu2^2 of the size of C1 = 1e-4.
``masks`` scales a face disc, a hair crescent and a mouth blob to the frame (variants: no hair at all, hair everywhere).

Statements.  The fp64 statement and the fp32 CPU statement are the project's own lines: losses.l1_loss / losses.ssim,
losses.face_loss_torch, train_stages.mouth_loss with _lips_mask, l1 + lambda (1 - ssim).  ``ssim_map`` restates the lines
of losses.ssim without the final mean; the per-pixel terms are used for the bars only.

Bars.  Nothing is measured on the code under test.  FACTOR = 4 and eps32 = 2^-23 as in deepspeech_helpers.bar,
track_helpers and photo_helpers.
  tensors   |operator - fp64| <= 4 max(e32, eps32 max|fp64|) over all elements, e32 the largest error of the fp32 CPU
            statement's autograd against the fp64 one.
  scalars   a single fp32 number can be right by accident (on a smooth 33x49 pair the fp32 SSIM is 5e-8 off while its
            pixels are 8e-4 off), so a mean of per-pixel terms t gets
                4 max(mean|t32 - t64|, eps32 mean|t64|) + d (eps32 / 2) mean|t64|
            with eps32 / 2 = 2^-24 the most one rounded addition loses and d the number of additions on the longest
            path of the kernels' reduction of n partial sums (``reduction_depth``): the workgroup's sum of 256 values is
            a butterfly over 64 lanes (6) and three additions of the waves' sums (9 together, one more than a 256-wide
            tree), the partial sums go down a lane-strided chain of ceil(n / 64) additions and another butterfly (6),
            and one division ends it:
                d = 9 + ceil(n / 64) + 6 + 1.
            n = 3 tiles for SSIM and L1 of the face kernels (C tiles for the generic kernel, whose partial sums torch.sum
            adds up as a tree no deeper than that chain and butterfly), tiles for the alpha / attention sums, and the
            number of elements for the extra term (no workgroup stage: ceil(n / 64) + 6 + 1).
            The loss's bar is the sum of its terms' bars weighted with |w_k|.
            (With a whole eps32 per addition the noise pair's SSIM bar at 75x131 would be 4.3e-6, above the 3.4e-6 =
            0.1 / (C H W) that test_loss_helpers_host.py demands of it; with the unit roundoff it is 3.3e-6.  The tighter
            form asks more of the kernels, not less.)
"""
import functools
import math

import torch

from instag_amd import losses
from instag_amd.train_stages import _lips_mask, mouth_loss

EPS32 = 2.0 ** -23
FACTOR = 4.0
TS, RAD = 16, 5                   # csrc/ssim.hip: tile side, window radius
SHAPES = ((1, 1), (5, 7), (11, 11),           # inside the window
          (15, 16),                           # a ragged single tile
          (16, 16),                           # exactly one tile
          (17, 16), (16, 33),                 # one row / one column in the next tile
          (26, 26),                           # the halo size
          (33, 49), (75, 131))                # several tiles, ragged both ways
KINDS = ("noise", "smooth", "composite", "dark")
BG = (0.25, 0.75, 0.5)
GENERIC_UPSTREAMS = ((1.0, -3.0), (1.0, None), (None, 1.0))       # on (l1, ssim)
FACE_UPSTREAMS = ((1.0, None), (None, 1.0), (1.5, -0.5))          # on (loss, Ll1)


def sid(shape):
    return f"{shape[0]}x{shape[1]}"


def tiles(H, W):
    return ((H + TS - 1) // TS) * ((W + TS - 1) // TS)


def reduction_depth(n, workgroup=True):
    return (9 if workgroup else 0) + math.ceil(n / 64) + 6 + 1


# ---- inputs -----------------------------------------------------------------------------------------------------------
def _coords(H, W):
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    u, v = (yy + 0.5) / H - 0.5, (xx + 0.5) / W - 0.5
    return yy, xx, u, v, torch.sqrt(u * u + v * v)


def background(C, dtype=torch.float32):
    return torch.tensor([BG[c % 3] for c in range(C)], dtype=dtype)


def zones(H, W):
    """The composite's zones as boolean [H, W] masks: disc, bleed, same, strip (disjoint, covering the frame)."""
    yy, _, _, _, r = _coords(H, W)
    strip = yy >= H - (H + 1) // 6
    disc = (r < 0.30) & ~strip
    bleed = (r >= 0.30) & (r < 0.40) & ~strip
    same = (r >= 0.40) & ~strip
    return {"disc": disc, "bleed": bleed, "same": same, "strip": strip}


def _smooth(C, H, W, g):
    yy, xx, _, _, _ = _coords(H, W)
    px, py = (110.0, 70.0, 150.0), (140.0, 90.0, 50.0)
    base = torch.stack([0.5 + 0.35 * torch.sin(2 * math.pi * xx / px[c % 3] + c) * torch.cos(2 * math.pi * yy / py[c % 3] - c)
                        for c in range(C)])
    ripple = torch.sin(2 * math.pi * (xx / 31.0 + yy / 47.0))
    x = (base + 0.01 * torch.randn(C, H, W, generator=g, dtype=torch.float64)).clamp(0, 1)
    y = (base + 0.03 * ripple[None]).clamp(0, 1)
    return x, y


def pair(kind, C, H, W, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 17)
    if kind == "noise":
        x = torch.rand(C, H, W, generator=g, dtype=torch.float64)
        y = (x + 0.2 * torch.randn(C, H, W, generator=g, dtype=torch.float64)).clamp(0, 1)
    elif kind == "smooth":
        x, y = _smooth(C, H, W, g)
    elif kind == "dark":
        x, y = _smooth(C, H, W, g)
        x, y = 0.029 * x, 0.029 * y
    elif kind == "composite":
        sx, sy = _smooth(C, H, W, g)
        sx = (sy + 0.02 * torch.randn(C, H, W, generator=g, dtype=torch.float64)).clamp(0, 1)
        z = zones(H, W)
        _, xx, _, _, _ = _coords(H, W)
        bg = background(C, torch.float64)[:, None, None].expand(C, H, W)
        x = torch.where(z["disc"][None], sx, bg)
        y = torch.where(z["disc"][None], sy, bg)
        x = torch.where(z["bleed"][None], bg - 0.02 * torch.rand(C, H, W, generator=g, dtype=torch.float64), x)
        wave = torch.stack([torch.sin(2 * math.pi * xx / 9.0 + c) for c in range(C)])
        wave_y = torch.stack([torch.sin(2 * math.pi * xx / 9.0 + c + 0.8) for c in range(C)])
        x = torch.where(z["strip"][None], (wave > 0).double(), x)
        y = torch.where(z["strip"][None], (wave_y > 0).double(), y)
    else:
        raise ValueError(kind)
    return x.float(), y.float()


def masks(H, W, variant="default"):
    """face disc, hair crescent over it, mouth blob below the centre -> bool [H, W] each."""
    _, _, u, v, r = _coords(H, W)
    face = r < 0.30
    hair = (r < 0.40) & (u < -0.10) & ~face
    mouth = torch.sqrt((u - 0.15) ** 2 + v ** 2) < 0.12
    if variant == "no_hair":
        hair = torch.zeros_like(hair)
    elif variant == "all_hair":
        hair = torch.ones_like(hair)
    elif variant != "default":
        raise ValueError(variant)
    return face, hair, mouth


def default_lips(H, W):
    r0, c0 = int(0.55 * H), int(0.3 * W)
    return (r0, max(int(0.75 * H), r0 + 1), c0, max(int(0.7 * W), c0 + 1))            # never empty


def frozen_face(H, W, variant="default"):
    """Pixels the background overwrites under hair_mask_iter."""
    return masks(H, W, variant)[1]


def frozen_mouth(H, W):
    """Pixels the background overwrites in the mouth mode: lips != mouth."""
    mouth = masks(H, W)[2]
    return _lips_mask(mouth, default_lips(H, W)) ^ mouth


# ---- statements ---------------------------------------------------------------------------------------------------------
def ssim_map(img1, img2, window_size=11):
    """The lines of losses.ssim without the final mean."""
    import torch.nn.functional as F
    squeeze = img1.dim() == 3
    if squeeze:
        img1, img2 = img1.unsqueeze(0), img2.unsqueeze(0)
    ch = img1.size(-3)
    w = losses._window(window_size, ch, img1.device, img1.dtype)
    pad = window_size // 2
    mu1 = F.conv2d(img1, w, padding=pad, groups=ch)
    mu2 = F.conv2d(img2, w, padding=pad, groups=ch)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1 = F.conv2d(img1 * img1, w, padding=pad, groups=ch) - mu1_sq
    s2 = F.conv2d(img2 * img2, w, padding=pad, groups=ch) - mu2_sq
    s12 = F.conv2d(img1 * img2, w, padding=pad, groups=ch) - mu12
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu12 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return m[0] if squeeze else m


class Term:
    """One mean of per-element terms of a loss: value = sum(t) / denom, entering the loss with weight w; n partial sums."""

    def __init__(self, w, t, denom, n, workgroup=True):
        self.w, self.t, self.denom, self.d = float(w), t.detach().double(), float(denom), reduction_depth(n, workgroup)


def scalar_bar(t32: Term, t64: Term):
    mean64 = float(t64.t.abs().sum()) / t64.denom
    spread = float((t32.t - t64.t).abs().sum()) / t64.denom
    return FACTOR * max(spread, EPS32 * mean64) + t64.d * 0.5 * EPS32 * mean64


def tensor_bar(g32, g64):
    e32 = float((g32.double() - g64).abs().max()) if g64.numel() else 0.0
    floor = EPS32 * (float(g64.abs().max()) if g64.numel() else 0.0)
    return e32, floor, FACTOR * max(e32, floor)


class Case:
    """One loss call: ``leaves`` (name -> float32 tensor that takes a gradient), ``consts`` (name -> tensor or plain
    value), ``statement(args, dtype)`` -> (outputs, terms) the project's lines on the CPU, ``operator(args)`` ->
    outputs the code under test, ``out_names`` what each output is: the name of one term, or the weighted sum of all of
    them ("loss")."""

    def __init__(self, name, leaves, consts, statement, operator, out_names, upstreams):
        self.name, self.leaves, self.consts = name, leaves, consts
        self.statement, self.operator, self.out_names, self.upstreams = statement, operator, out_names, upstreams
        self._ref = None

    def args(self, device, dtype):
        """Fresh leaves and constants on ``device``: floating tensors in ``dtype``."""
        conv = lambda t: t.to(device, dtype) if torch.is_tensor(t) and t.is_floating_point() else (
            t.to(device) if torch.is_tensor(t) else t)
        leaves = {k: conv(v).detach().clone().requires_grad_(True) for k, v in self.leaves.items()}
        return leaves, {k: conv(v) for k, v in self.consts.items()}

    @staticmethod
    def _grads(outs, leaves, upstream, retain):
        tot = sum(u * o for u, o in zip(upstream, outs) if u is not None)
        gs = torch.autograd.grad(tot, list(leaves.values()), allow_unused=True, retain_graph=retain)
        return {k: (torch.zeros_like(v) if g is None else g).detach() for (k, v), g in zip(leaves.items(), gs)}

    def reference(self):
        """fp64 and fp32 CPU statements, computed once: values, scalar bars, gradients per upstream."""
        if self._ref is None:
            ref = {}
            for dt in (torch.float64, torch.float32):
                leaves, consts = self.args("cpu", dt)
                outs, terms = self.statement({**leaves, **consts}, dt)
                grads = [self._grads(outs, leaves, u, True) for u in self.upstreams]
                ref[dt] = ([float(o.detach()) for o in outs], terms, grads)
            bars = {k: scalar_bar(ref[torch.float32][1][k], t) for k, t in ref[torch.float64][1].items()}
            w = {k: abs(t.w) for k, t in ref[torch.float64][1].items()}
            out_bars = []
            for name in self.out_names:
                out_bars.append(bars[name] if name in bars else sum(w[k] * bars[k] for k in bars))
            self._ref = {"out64": ref[torch.float64][0], "out32": ref[torch.float32][0], "out_bars": out_bars,
                         "term_bars": bars, "grads64": ref[torch.float64][2], "grads32": ref[torch.float32][2]}
        return self._ref

    def run(self, device, upstream):
        """The operator on ``device`` in float32 -> (outputs as tensors, gradients by leaf name)."""
        leaves, consts = self.args(device, torch.float32)
        outs = self.operator({**leaves, **consts})
        grads = self._grads(outs, leaves, upstream, False)
        return [o.detach() for o in outs], grads


def compare(case, device, record=None):
    """Runs ``case`` on ``device`` under each of its upstream gradients and holds values and gradients to their bars;
    prints operator, e32 and bar of every comparison before it asserts.  -> the largest operator / max(e32, floor)."""
    ref = case.reference()
    worst, failures = 0.0, []
    for ui, up in enumerate(case.upstreams):
        outs, grads = case.run(device, up)
        tag = f"{case.name} up={up}"
        if ui == 0:
            for name, o, v64, v32, bar in zip(case.out_names, outs, ref["out64"], ref["out32"], ref["out_bars"]):
                err = abs(float(o) - v64)
                print(f"{case.name} {name}: operator {err:.3e} e32 {abs(v32 - v64):.3e} bar {bar:.3e} fp64 {v64:.6e}")
                if record is not None:
                    record.setdefault(case.name, {})[name] = {"operator": err, "e32": abs(v32 - v64), "bar": bar, "fp64": v64}
                assert o.dtype == torch.float32 and math.isfinite(float(o)), (tag, name)
                if not err <= bar:
                    failures.append((tag, name, err, bar))
        for k, got in grads.items():
            g64, g32 = ref["grads64"][ui][k], ref["grads32"][ui][k]
            assert tuple(got.shape) == tuple(g64.shape) and got.dtype == torch.float32, (tag, k)
            assert bool(torch.isfinite(got).all()), (tag, k)
            e32, floor, bar = tensor_bar(g32, g64)
            err = float((got.double().cpu() - g64).abs().max()) if g64.numel() else 0.0
            ratio = err / max(e32, floor) if max(e32, floor) > 0 else 0.0
            print(f"{tag} d_{k}: operator {err:.3e} e32 {e32:.3e} bar {bar:.3e} max|fp64| {floor / EPS32:.3e} "
                  f"ratio {ratio:.2f}")
            if record is not None:             # per gradient the upstream that came closest to its bar
                slot = record.setdefault(case.name, {})
                if "d_" + k not in slot or ratio > slot["d_" + k]["ratio"]:
                    slot["d_" + k] = {"operator": err, "e32": e32, "bar": bar, "max_fp64": floor / EPS32,
                                      "ratio": ratio, "upstream": list(up)}
            if k == "image":
                worst = max(worst, ratio)
            if not err <= bar:
                failures.append((tag, "d_" + k, err, bar))
    assert not failures, failures
    return worst


# ---- the cases ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def generic_case(kind, C, H, W):
    x, y = pair(kind, C, H, W)
    n = C * tiles(H, W)

    def statement(a, dt):
        outs = (losses.l1_loss(a["image"], a["gt"]), losses.ssim(a["image"], a["gt"]))
        with torch.no_grad():
            terms = {"l1": Term(1.0, (a["image"] - a["gt"]).abs(), x.numel(), n),
                     "ssim": Term(1.0, ssim_map(a["image"], a["gt"]), x.numel(), n)}
        return outs, terms

    return Case(f"generic {kind} C={C} {H}x{W}", {"image": x}, {"gt": y}, statement,
                lambda a: losses.l1_and_ssim(a["image"], a["gt"]), ("l1", "ssim"), GENERIC_UPSTREAMS)


def _image_terms(xg, yg, lam, H, W):
    n = 3 * tiles(H, W)
    return {"l1": Term(1.0, (xg - yg).abs(), xg.numel(), n), "ssim": Term(lam, ssim_map(xg, yg), xg.numel(), n)}


@functools.lru_cache(maxsize=None)
def plain_case(kind, H, W, lam=0.2):
    x, y = pair(kind, 3, H, W)

    def statement(a, dt):
        l1 = losses.l1_loss(a["image"], a["gt"])
        outs = (l1 + lam * (1.0 - losses.ssim(a["image"], a["gt"])), l1)
        with torch.no_grad():
            terms = _image_terms(a["image"], a["gt"], lam, H, W)
        return outs, terms

    return Case(f"plain {kind} {H}x{W}", {"image": x}, {"gt": y}, statement,
                lambda a: losses.plain_loss_fused(a["image"], a["gt"], lam), ("loss", "l1"), FACE_UPSTREAMS)


@functools.lru_cache(maxsize=None)
def face_case(kind, H, W, alpha=True, attn=True, lips="default", n_extra=1, hair_mask_iter=False, variant="default",
              lam=0.2, w_lips=5e-3):
    """losses.face_loss against losses.face_loss_torch.  ``lips``: None, "default" or (row0, row1, col0, col1);
    ``n_extra``: 0 for no extra term.  The weights are the train step's but for w_extra, which is 0.01 so that the term
    shows in the loss."""
    x, y = pair(kind, 3, H, W)
    g = torch.Generator().manual_seed(H * 1000 + W)
    face, hair, mouth = masks(H, W, variant)
    rect = default_lips(H, W) if lips == "default" else lips
    leaves = {"image": x}
    if alpha:
        leaves["alpha"] = torch.rand(1, H, W, generator=g)
    if attn:
        leaves["attn"] = torch.rand(3, H, W, generator=g)
    if n_extra:
        leaves["extra"] = torch.rand(n_extra, generator=g) - 0.3
    consts = {"gt": y, "face": face, "hair": hair, "mouth": mouth, "bg": background(3)}
    kw = dict(lambda_dssim=lam, w_alpha=1e-3, w_attn=1e-4, w_extra=1e-2, hair_mask_iter=hair_mask_iter, w_lips=w_lips)
    nt = tiles(H, W)

    def call(fn, a):
        return fn(a["image"], a["gt"], a["face"], a["hair"], a["mouth"], a["bg"], alpha=a.get("alpha"), attn=a.get("attn"),
                  lips_rect=rect, extra=a.get("extra"), **kw)

    def statement(a, dt):
        outs = call(losses.face_loss_torch, a)
        with torch.no_grad():
            head = a["face"] | a["hair"]
            keep = head & ~a["mouth"]
            bg3 = a["bg"][:, None, None]
            xg = a["image"]
            if hair_mask_iter:
                keep = keep & ~a["hair"]
                xg = torch.where(a["hair"][None], bg3.expand_as(xg), xg)
            yg = torch.where(keep[None], a["gt"], bg3.expand_as(a["gt"]))
            terms = _image_terms(xg, yg, lam, H, W)
            if n_extra:
                terms["extra"] = Term(kw["w_extra"], a["extra"], 1, n_extra, workgroup=False)
            if alpha:
                hm = head.to(dt)
                terms["alpha_in"] = Term(1e-3, (1 - a["alpha"]) * hm, H * W, nt)
                terms["alpha_out"] = Term(1e-3, a["alpha"] * (1 - hm), H * W, nt)
            if attn:
                if rect is not None:
                    r0, r1, c0, c1 = rect
                    sl = a["attn"][1, r0:r1, c0:c1]
                    terms["lips"] = Term(w_lips, sl, max(sl.numel(), 1), nt)
                if not hair_mask_iter:
                    cnt = max(int(a["hair"].sum()), 1)
                    hf = a["hair"].to(dt)
                    terms["hair1"] = Term(1e-4, a["attn"][1] * hf, cnt, nt)
                    terms["hair0"] = Term(1e-4, a["attn"][0] * hf, cnt, nt)
        return outs, terms

    on = "".join(c for c, f in zip("aAleh", (alpha, attn, attn and rect is not None, n_extra, hair_mask_iter)) if f)
    name = f"face {kind} {H}x{W} [{on or '-'}]"
    if lips not in (None, "default"):
        name += f" lips={tuple(lips)}"
    if n_extra > 1:
        name += f" extra={n_extra}"
    if variant != "default":
        name += " " + variant
    return Case(name, leaves, consts, statement, lambda a: call(losses.face_loss, a), ("loss", "l1"), FACE_UPSTREAMS)


@functools.lru_cache(maxsize=None)
def mouth_case(kind, H, W, warm=True, way="p_xyz", lam=0.2):
    """losses.mouth_loss_fused against train_stages.mouth_loss.  ``way``: how the alignment term arrives -- "p_xyz" (the
    positions), "p_raw" (the head's raw output the positions are 1e-2 of) or "extra" (already weighted partial sums)."""
    x, y = pair(kind, 3, H, W)
    g = torch.Generator().manual_seed(H * 1000 + W + 1)
    mouth = masks(H, W)[2]
    rect = torch.tensor(default_lips(H, W), dtype=torch.int32)
    leaves = {"image": x, "alpha": torch.rand(1, H, W, generator=g)}
    shape = {"p_xyz": (37, 3), "p_raw": (37, 5), "extra": (70,)}[way]
    leaves["p"] = torch.randn(*shape, generator=g) * (1e-2 if way == "p_xyz" else 1.0) * (1e-3 if way == "extra" else 1.0)
    consts = {"gt": y, "mouth": mouth, "rect": rect, "bg": background(3)}

    def statement(a, dt):
        p_xyz = None if way == "extra" else (a["p"] if way == "p_xyz" else a["p"][:, :3] * 1e-2)
        lm = _lips_mask(a["mouth"], a["rect"])
        loss, l1 = mouth_loss(a["image"], a["alpha"], a["gt"], a["mouth"], lm, a["bg"], p_xyz, warm=warm, lambda_dssim=lam)
        if way == "extra":
            loss = loss + a["p"].sum()
        with torch.no_grad():
            bg3 = a["bg"][:, None, None]
            yg = torch.where(a["mouth"][None], a["gt"], bg3.expand_as(a["gt"]))
            xg = torch.where((lm ^ a["mouth"])[None], bg3.expand_as(a["image"]), a["image"])
            terms = _image_terms(xg, yg, lam, H, W)
            if way == "extra":
                terms["extra"] = Term(1.0, a["p"], 1, a["p"].numel(), workgroup=False)
            elif warm:
                terms["extra"] = Term(1e-5, p_xyz.abs(), p_xyz.numel(), p_xyz.numel())
            if warm:
                lf = lm.to(dt)
                terms["alpha_in"] = Term(1e-3, (1 - a["alpha"]) * lf, H * W, tiles(H, W))
                terms["alpha_out"] = Term(1e-3, a["alpha"] * (1 - lf), H * W, tiles(H, W))
        return (loss, l1), terms

    def operator(a):
        kw = {way: a["p"]}
        return losses.mouth_loss_fused(a["image"], a["alpha"], a["gt"], a["mouth"], a["rect"], a["bg"], warm=warm,
                                       lambda_dssim=lam, **kw)

    return Case(f"mouth {kind} {H}x{W} warm={int(warm)} {way}", leaves, consts, statement, operator, ("loss", "l1"),
                FACE_UPSTREAMS)
