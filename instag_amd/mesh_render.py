"""Refine tracked poses photometrically: the 3DMM mesh renderer on the device (csrc/mesh_render.hip) and the two fits.

After the landmark fit (track.py) the reference's tracker fits a texture and SH lighting on 32 frames
(face_tracker.py:207-286) and then refits expression, rotation, translation and light of every frame against the image,
32 frames at a time with a temporal Laplacian (:288-406).  Both render the whole 3DMM mesh through pytorch3d
(render_3dmm.py).  Here the renderer is this project's own statement of what ``Render_3DMM`` asks pytorch3d for, in plain
torch (``*_torch``: any device, fp32 or fp64; the definition, and the reference of the GPU tests), and HIP kernels that
compute the same (``MeshRenderer``).  Parity with pytorch3d itself is not pinned.

The statement.  Vertex stage: vertex normals through ``vert_tris`` used literally (a vertex normal is the normalised sum
of the unit normals of its M listed triangles, an index listed twice counting twice), nine SH basis values, colour =
texture * (Y @ gamma) with 0.8 added to band 0.  Screen: u = -f X / Z + W / 2, v = f Y / Z + H / 2 (project_torch's
pixel position), depth z = -Z; pixel (i, j) has its centre at (j + 0.5, i + 0.5); every 2-D quantity below is in units of
s = 2 / min(H, W) per pixel (pytorch3d's NDC scale).  Per pixel and face: edge functions, barycentrics, the smallest
squared point-segment distance, clipped barycentrics, depth; a face is a candidate when |area| > 1e-8, its largest
vertex depth >= 0, pz >= 0 and the pixel is inside or within blur_radius; the K = 2 candidates of smallest pz are kept
(ties: lower face index).  Blend: pytorch3d's softmax blend.  The selection is not differentiated; given the face ids
everything is differentiable in the screen vertices and the vertex colours, and autograd of the statement defines the
gradient.

Stated deviation: for even, square frames the screen above is exactly the camera render_3dmm.py:113-126 builds.  For
other sizes the reference's renderer and its landmark projection disagree with each other; the landmark projection is
kept.  W must be even.

    model = Face3DMM.load("data_utils/face_tracking/3DMM")      # + topology_info.npy
    renderer = MeshRenderer(model, focal, H, W)                  # renderer(rott_geo, texture, light) -> [B,H,W,4]
    params = track_identity(path, model, "cuda", photometric=True)
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np
import torch
import torch.nn.functional as Fn

from . import _lib
from ._lib import check_arg
from .track import Face3DMM, euler2rot_torch, landmarks_torch, project_torch

SIGMA = 1e-4
GAMMA = 1e-4
BLUR_RADIUS = math.log(1.0 / 1e-4 - 1.0) * SIGMA / 18.0
ZNEAR, ZFAR, EPS = 0.01, 20.0, 1e-10
K_FACES = 2
AREA_EPS = 1e-8            # a face of smaller |area| is never drawn; a segment of smaller squared length is a point
BARY_EPS = 1e-5

# Illumination_layer's constants (render_3dmm.py:160-166)
_A0, _A1, _A2 = math.pi, 2 * math.pi / math.sqrt(3.0), 2 * math.pi / math.sqrt(8.0)
_C0, _C1, _C2 = 1 / math.sqrt(4 * math.pi), math.sqrt(3.0) / math.sqrt(4 * math.pi), 3 * math.sqrt(5.0) / math.sqrt(12 * math.pi)
_D0 = 0.5 / math.sqrt(3.0)


def blur_radius_of(sigma):
    return math.log(1.0 / 1e-4 - 1.0) * sigma / 18.0


# ---- the model's full mesh ---------------------------------------------------------------------------------------------
def geometry_torch(model: Face3DMM, id_para, exp_para):
    """forward_geo (facemodel.py:140-148): [B,I], [B,E] -> [B,N,3]."""
    base_id, base_exp, mu, sig_id, sig_exp = model.full_tensors(id_para.device, id_para.dtype)
    geo = torch.mm(id_para * sig_id, base_id) + torch.mm(exp_para * sig_exp, base_exp) + mu
    return geo.reshape(-1, model.N, 3)


def geometry_sub_torch(model: Face3DMM, id_para, exp_para, sub_index):
    """forward_geo_sub (facemodel.py:122-138): the points ``sub_index`` only."""
    base_id, base_exp, mu, sig_id, sig_exp = model.full_tensors(id_para.device, id_para.dtype)
    sub_index = torch.as_tensor(sub_index, dtype=torch.int64, device=id_para.device)
    sel = torch.cat((3 * sub_index.unsqueeze(1), 3 * sub_index.unsqueeze(1) + 1, 3 * sub_index.unsqueeze(1) + 2), dim=1).reshape(-1)
    geo = torch.mm(id_para * sig_id, base_id[:, sel]) + torch.mm(exp_para * sig_exp, base_exp[:, sel]) + mu[sel]
    return geo.reshape(-1, sub_index.shape[0], 3)


def texture_torch(model: Face3DMM, tex_para):
    """forward_tex (facemodel.py:150-153): [B,tex_dim] -> [B,N,3]."""
    base_tex, mu_tex, sig_tex = model.texture_tensors(tex_para.device, tex_para.dtype)
    return (torch.mm(tex_para * sig_tex, base_tex) + mu_tex).reshape(-1, model.N, 3)


def rott_torch(geometry, euler, trans):
    """forward_rott (util.py:86-89): R p + t, [B,N,3]."""
    return (torch.bmm(euler2rot_torch(euler), geometry.permute(0, 2, 1)) + trans[:, :, None]).permute(0, 2, 1)


def color_loss_torch(pred, gt, mask):
    """cal_col_loss (util.py:103-109): pred, gt [B,H,W,3], mask [B,H,W]."""
    loss = torch.sum(torch.square(pred - gt), 3) * mask / 255
    loss = torch.sum(loss, dim=(1, 2)) / torch.sum(mask, dim=(1, 2))
    return torch.mean(loss)


def lap_loss_torch(x):
    """cal_lap_loss (util.py:57-71) of one tensor with weight 1: x [P,F], the kernel (-0.5, 1, -0.5) along the frame axis."""
    kernel = torch.tensor((-0.5, 1.0, -0.5), dtype=x.dtype, device=x.device).view(1, 1, 3)
    return torch.mean(Fn.conv1d(x.reshape(-1, 1, x.shape[-1]), kernel) ** 2)


# ---- vertex stage ------------------------------------------------------------------------------------------------------
def vertex_normals_torch(rott_geo, tris, vert_tris):
    """compute_normal (render_3dmm.py:103-111)."""
    v1 = torch.index_select(rott_geo, 1, tris[:, 0])
    v2 = torch.index_select(rott_geo, 1, tris[:, 1])
    v3 = torch.index_select(rott_geo, 1, tris[:, 2])
    nnorm = torch.cross(v2 - v1, v3 - v1, dim=2)
    tri_normal = Fn.normalize(nnorm, dim=2)
    v_norm = tri_normal[:, vert_tris, :].sum(2)
    return v_norm / v_norm.norm(dim=2).unsqueeze(2)


def sh_basis_torch(normals):
    """The nine basis values of Illumination_layer (render_3dmm.py:168-184): [..., 3] -> [..., 9]."""
    nx, ny, nz = normals[..., 0], normals[..., 1], normals[..., 2]
    return torch.stack((torch.ones_like(nx) * _A0 * _C0, -_A1 * _C1 * ny, _A1 * _C1 * nz, -_A1 * _C1 * nx,
                        _A2 * _C2 * nx * ny, -_A2 * _C2 * ny * nz, _A2 * _C2 * _D0 * (3 * nz.pow(2) - 1),
                        -_A2 * _C2 * nx * nz, _A2 * _C2 * 0.5 * (nx.pow(2) - ny.pow(2))), dim=-1)


def illumination_torch(texture, normals, light):
    """Illumination_layer (render_3dmm.py:150-188): texture [B,V,3], normals [B,V,3], light [B,27] -> colours [B,V,3]."""
    gamma = light.view(-1, 3, 9).clone()
    gamma[:, :, 0] += 0.8
    gamma = gamma.permute(0, 2, 1)
    return texture * sh_basis_torch(normals).bmm(gamma)


def vertex_stage_torch(rott_geo, texture, light, tris, vert_tris):
    return illumination_torch(texture, vertex_normals_torch(rott_geo, tris, vert_tris), light)


# ---- screen ------------------------------------------------------------------------------------------------------------
def screen_torch(rott_geo, focal, H, W):
    """[B,V,3] camera-space points -> [B,V,3] = (u, v, z): pixel position of project_torch with cx = W/2, cy = H/2,
    depth z = -Z."""
    X, Y, Z = rott_geo[..., 0], rott_geo[..., 1], rott_geo[..., 2]
    return torch.stack((-(focal * X) / Z + W / 2.0, (focal * Y) / Z + H / 2.0, -Z), dim=-1)


def _check_size(H, W):
    if W % 2 or H < 1 or W < 2:
        raise ValueError(f"the mesh renderer needs an even image width (got {H} x {W})")


def _edge(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def _seg_dist2(px, py, ax, ay, bx, by):
    """Squared distance of p to the segment a-b; a segment of squared length <= 1e-8 counts as its end point b."""
    dx, dy = bx - ax, by - ay
    l2 = dx * dx + dy * dy
    short = l2 <= AREA_EPS
    t = (dx * (px - ax) + dy * (py - ay)) / torch.where(short, torch.ones_like(l2), l2)
    t = t.clamp(0.0, 1.0)
    # the end point itself at t = 1 (a + 0 d is a already): two edges whose nearest point is their shared corner tie exactly
    qx, qy = torch.where(t >= 1.0, bx + 0.0 * t, ax + t * dx), torch.where(t >= 1.0, by + 0.0 * t, ay + t * dy)
    d_seg = (px - qx) ** 2 + (py - qy) ** 2
    d_end = (px - bx) ** 2 + (py - by) ** 2
    return torch.where(short, d_end, d_seg)


def face_terms_torch(px, py, v0, v1, v2):
    """px, py and the three vertices (x, y in units of s, depth z) broadcast against each other ->
    dict(area, w [3], inside, dist, bary [3] (clipped), pz)."""
    area = _edge(v2[0], v2[1], v0[0], v0[1], v1[0], v1[1])
    safe = torch.where(area.abs() > AREA_EPS, area, torch.ones_like(area))
    w0 = _edge(px, py, v1[0], v1[1], v2[0], v2[1]) / safe
    w1 = _edge(px, py, v2[0], v2[1], v0[0], v0[1]) / safe
    w2 = _edge(px, py, v0[0], v0[1], v1[0], v1[1]) / safe
    inside = (w0 > 0) & (w1 > 0) & (w2 > 0)
    d01 = _seg_dist2(px, py, v0[0], v0[1], v1[0], v1[1])
    d12 = _seg_dist2(px, py, v1[0], v1[1], v2[0], v2[1])
    d20 = _seg_dist2(px, py, v2[0], v2[1], v0[0], v0[1])
    d = torch.minimum(torch.minimum(d01, d12), d20)
    dist = torch.where(inside, -d, d)
    c0, c1, c2 = w0.clamp(0.0, 1.0), w1.clamp(0.0, 1.0), w2.clamp(0.0, 1.0)
    s = (c0 + c1 + c2).clamp(min=BARY_EPS)
    b0, b1, b2 = c0 / s, c1 / s, c2 / s
    pz = b0 * v0[2] + b1 * v1[2] + b2 * v2[2]
    return dict(area=area, w=(w0, w1, w2), inside=inside, dist=dist, bary=(b0, b1, b2), pz=pz, edges=(d01, d12, d20))


def _pixel_centres(H, W, s, dtype, device):
    py = (torch.arange(H, dtype=dtype, device=device) + 0.5) * s
    px = (torch.arange(W, dtype=dtype, device=device) + 0.5) * s
    return px, py


def candidates_dense_torch(screen, tris, H, W, blur_radius=BLUR_RADIUS, rows=None):
    """The statement's per-pixel, per-face table for the image rows ``rows`` (default all): dict(cand [B,h,W,T] bool,
    pz, dist, inside).  Dense over the faces: for tests and small images."""
    s = 2.0 / min(H, W)
    px, py = _pixel_centres(H, W, s, screen.dtype, screen.device)
    if rows is not None:
        py = py[rows[0]:rows[1]]
    px, py = px.view(1, 1, -1, 1), py.view(1, -1, 1, 1)
    vs = []
    for k in range(3):
        p = screen[:, tris[:, k]]                                   # [B,T,3]
        vs.append((p[..., 0].mul(s)[:, None, None, :], p[..., 1].mul(s)[:, None, None, :], p[..., 2][:, None, None, :]))
    t = face_terms_torch(px, py, *vs)
    zmax = torch.maximum(torch.maximum(vs[0][2], vs[1][2]), vs[2][2])
    cand = (t["area"].abs() > AREA_EPS) & (zmax >= 0) & (t["pz"] >= 0) & (t["inside"] | (t["dist"] < blur_radius))
    return dict(cand=cand, pz=t["pz"], dist=t["dist"], inside=t["inside"])


@torch.no_grad()
def select_torch(screen, tris, H, W, blur_radius=BLUR_RADIUS, K=K_FACES, chunk_rows=16):
    """Face ids [B,H,W,K] int64 (-1: empty slot): per pixel the K candidates of smallest pz, ties to the lower face index."""
    _check_size(H, W)
    out = []
    for r0 in range(0, H, chunk_rows):
        t = candidates_dense_torch(screen, tris, H, W, blur_radius, (r0, min(H, r0 + chunk_rows)))
        pz = torch.where(t["cand"], t["pz"], torch.full_like(t["pz"], float("inf")))
        val, idx = torch.sort(pz, dim=-1, stable=True)               # stable: equal pz keep ascending face index
        val, idx = val[..., :K], idx[..., :K]
        if val.shape[-1] < K:
            pad = K - val.shape[-1]
            val = torch.cat((val, torch.full_like(val[..., :1], float("inf")).expand(*val.shape[:-1], pad)), dim=-1)
            idx = torch.cat((idx, torch.zeros_like(idx[..., :1]).expand(*idx.shape[:-1], pad)), dim=-1)
        out.append(torch.where(torch.isinf(val), torch.full_like(idx, -1), idx))
    return torch.cat(out, dim=1)


def blend_torch(screen, colours, tris, ids, H, W, sigma=SIGMA, gamma=GAMMA, znear=ZNEAR, zfar=ZFAR, background=(0.0, 0.0, 0.0),
                eps=EPS, return_terms=False):
    """screen [B,V,3] (u, v, z), colours [B,V,3], ids [B,H,W,K] -> [B,H,W,4] = clamp((rgb, alpha), 0, 255): the softmax
    blend of the K faces of every pixel.  Differentiable in screen and colours."""
    _check_size(H, W)
    B = screen.shape[0]
    s = 2.0 / min(H, W)
    m = ids >= 0
    face = tris[ids.clamp(min=0)]                                   # [B,H,W,K,3]
    b_idx = torch.arange(B, device=screen.device).view(B, 1, 1, 1)
    px, py = _pixel_centres(H, W, s, screen.dtype, screen.device)
    px, py = px.view(1, 1, -1, 1), py.view(1, -1, 1, 1)
    vs, cols = [], []
    for k in range(3):
        p = screen[b_idx, face[..., k]]                             # [B,H,W,K,3]
        vs.append((p[..., 0] * s, p[..., 1] * s, p[..., 2]))
        cols.append(colours[b_idx, face[..., k]])
    t = face_terms_torch(px, py, *vs)
    zero = torch.zeros_like(t["pz"])
    prob = torch.where(m, torch.sigmoid(-t["dist"] / sigma), zero)
    alpha = 1.0 - torch.prod(1.0 - prob, dim=-1)
    zinv = torch.where(m, (zfar - t["pz"]) / (zfar - znear), zero)
    zmax = torch.max(zinv, dim=-1).values[..., None].clamp(min=eps)
    wn = prob * torch.exp((zinv - zmax) / gamma)
    delta = torch.exp((eps - zmax) / gamma).clamp(min=eps)
    b0, b1, b2 = t["bary"]
    colour = b0[..., None] * cols[0] + b1[..., None] * cols[1] + b2[..., None] * cols[2]    # [B,H,W,K,3]
    bg = torch.as_tensor(background, dtype=screen.dtype, device=screen.device)
    rgb = ((wn[..., None] * colour).sum(dim=-2) + delta * bg) / (wn.sum(dim=-1, keepdim=True) + delta)
    out = torch.cat((rgb, alpha[..., None]), dim=-1).clamp(0.0, 255.0)
    return (out, t) if return_terms else out


def render_torch(rott_geo, texture, light, tris, vert_tris, focal, H, W, sigma=SIGMA, gamma=GAMMA, blur_radius=None,
                 znear=ZNEAR, zfar=ZFAR, background=(0.0, 0.0, 0.0), eps=EPS, return_ids=False):
    """Render_3DMM.forward in this project's statement: [B,V,3], [B,V,3], [B,27] -> [B,H,W,4]."""
    blur_radius = blur_radius_of(sigma) if blur_radius is None else blur_radius
    colours = vertex_stage_torch(rott_geo, texture, light, tris, vert_tris)
    screen = screen_torch(rott_geo, focal, H, W)
    ids = select_torch(screen.detach(), tris, H, W, blur_radius)
    out = blend_torch(screen, colours, tris, ids, H, W, sigma, gamma, znear, zfar, background, eps)
    return (out, ids) if return_ids else out


# ---- the kernels -------------------------------------------------------------------------------------------------------
def _settings(r):
    a = _lib.MeshSettings()
    a.H, a.W, a.K = r.H, r.W, K_FACES
    a.sigma, a.gamma, a.blur_radius, a.znear, a.zfar, a.eps = r.sigma, r.gamma, r.blur_radius, r.znear, r.zfar, r.eps
    a.bg_r, a.bg_g, a.bg_b = r.background
    return a


def _f32c(t, what, device):
    if t.dtype != torch.float32 or t.device != device:
        raise ValueError(f"mesh_render: {what} must be a float32 tensor on {device}")
    return t.contiguous()


class _VertexStage(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r, rott_geo, texture, light):
        rott_geo, texture, light = (_f32c(t.detach(), n, r.device) for t, n in
                                    ((rott_geo, "rott_geo"), (texture, "texture"), (light, "light")))
        B, V = rott_geo.shape[0], rott_geo.shape[1]
        if rott_geo.shape != (B, r.V, 3) or texture.shape != (B, V, 3) or light.shape != (B, 27):
            raise ValueError(f"mesh_render: rott_geo [B,{r.V},3], texture [B,{r.V},3], light [B,27]")
        colours = torch.empty_like(texture)
        with torch.cuda.device(r.device):
            check_arg(_lib.lib().instag_mesh_vertex_forward(_lib.ptr(rott_geo), _lib.ptr(texture), _lib.ptr(light), _lib.ptr(r.tris),
                                                           _lib.ptr(r.vert_tris), B, V, r.T, r.M, _lib.ptr(colours),
                                                           _lib.current_stream()), "mesh_vertex_forward")
        ctx.r = r
        ctx.save_for_backward(rott_geo, texture, light)
        return colours

    @staticmethod
    def backward(ctx, d_colours):
        r = ctx.r
        rott_geo, texture, light = ctx.saved_tensors
        B, V = rott_geo.shape[0], rott_geo.shape[1]
        d_colours = _f32c(d_colours, "d_colours", r.device)
        d_geo, d_tex, d_light = torch.empty_like(rott_geo), torch.empty_like(texture), torch.empty_like(light)
        lib = _lib.lib()
        ws = torch.empty(int(lib.instag_mesh_vertex_backward_workspace_bytes(B, V)), dtype=torch.uint8, device=r.device)
        with torch.cuda.device(r.device):
            check_arg(lib.instag_mesh_vertex_backward(_lib.ptr(rott_geo), _lib.ptr(texture), _lib.ptr(light), _lib.ptr(r.tris),
                                                     _lib.ptr(r.vert_tris), _lib.ptr(d_colours), B, V, r.T, r.M, _lib.ptr(d_geo),
                                                     _lib.ptr(d_tex), _lib.ptr(d_light), _lib.ptr(ws), ws.numel(),
                                                     _lib.current_stream()), "mesh_vertex_backward")
        return None, d_geo, d_tex, d_light


class _Blend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r, screen, colours, ids):
        screen, colours = _f32c(screen.detach(), "screen", r.device), _f32c(colours.detach(), "colours", r.device)
        B = screen.shape[0]
        if screen.shape != (B, r.V, 3) or colours.shape != (B, r.V, 3) or ids.shape != (B, r.H, r.W, K_FACES):
            raise ValueError(f"mesh_render: screen [B,{r.V},3], colours [B,{r.V},3], ids [B,{r.H},{r.W},{K_FACES}]")
        if ids.dtype != torch.int32 or ids.device != r.device:
            raise ValueError("mesh_render: ids must be an int32 tensor on the renderer's device")
        ids = ids.contiguous()
        out = torch.empty(B, r.H, r.W, 4, dtype=torch.float32, device=r.device)
        s = _settings(r)
        with torch.cuda.device(r.device):
            check_arg(_lib.lib().instag_mesh_blend_forward(C.byref(s), _lib.ptr(screen), _lib.ptr(colours), _lib.ptr(r.tris),
                                                          _lib.ptr(ids), B, r.V, r.T, _lib.ptr(out), _lib.current_stream()),
                     "mesh_blend_forward")
        ctx.r = r
        ctx.save_for_backward(screen, colours, ids)
        return out

    @staticmethod
    def backward(ctx, d_out):
        r = ctx.r
        screen, colours, ids = ctx.saved_tensors
        d_out = _f32c(d_out, "d_out", r.device)
        d_screen, d_colours = torch.empty_like(screen), torch.empty_like(colours)      # (the entry point clears them)
        s = _settings(r)
        with torch.cuda.device(r.device):
            check_arg(_lib.lib().instag_mesh_blend_backward(C.byref(s), _lib.ptr(screen), _lib.ptr(colours), _lib.ptr(r.tris),
                                                           _lib.ptr(ids), _lib.ptr(d_out), screen.shape[0], r.V, r.T,
                                                           _lib.ptr(d_screen), _lib.ptr(d_colours), _lib.current_stream()),
                     "mesh_blend_backward")
        return None, d_screen, d_colours, None


class MeshRenderer:
    """Render_3DMM on a HIP device: ``renderer(rott_geo [B,V,3], texture [B,V,3], light [B,27]) -> [B,H,W,4]``, fp32,
    differentiable in all three inputs.  ``select`` and ``blend`` expose the two halves, ``vertex_stage`` the colours.
    The projection to the screen between them is screen_torch under autograd."""

    def __init__(self, model: Face3DMM, focal, H, W, device="cuda", sigma=SIGMA, gamma=GAMMA, blur_radius=None, znear=ZNEAR,
                 zfar=ZFAR, background=(0.0, 0.0, 0.0), eps=EPS):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("MeshRenderer runs on a HIP device; render_torch serves any other")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        _check_size(H, W)
        tris, vert_tris = model.topology_tensors("cpu")
        self.tris = tris.to(torch.int32).to(self.device).contiguous()
        self.vert_tris = vert_tris.to(torch.int32).to(self.device).contiguous()
        self.V, self.T, self.M = model.N, int(tris.shape[0]), int(vert_tris.shape[1])
        self.focal, self.H, self.W = float(focal), int(H), int(W)
        self.sigma, self.gamma = float(sigma), float(gamma)
        self.blur_radius = float(blur_radius_of(sigma) if blur_radius is None else blur_radius)
        self.znear, self.zfar, self.eps = float(znear), float(zfar), float(eps)
        self.background = tuple(float(x) for x in background)

    def vertex_stage(self, rott_geo, texture, light):
        return _VertexStage.apply(self, rott_geo, texture, light)

    def screen(self, rott_geo):
        return screen_torch(rott_geo, self.focal, self.H, self.W)

    @torch.no_grad()
    def select(self, screen):
        """Face ids [B,H,W,2] int32, -1 for an empty slot."""
        screen = _f32c(screen.detach(), "screen", self.device)
        B = screen.shape[0]
        if screen.shape != (B, self.V, 3):
            raise ValueError(f"mesh_render: screen [B,{self.V},3]")
        keys = torch.full((B, self.H, self.W, K_FACES), -1, dtype=torch.int64, device=self.device)
        ids = torch.empty(B, self.H, self.W, K_FACES, dtype=torch.int32, device=self.device)
        s = _settings(self)
        with torch.cuda.device(self.device):
            check_arg(_lib.lib().instag_mesh_select(C.byref(s), _lib.ptr(screen), _lib.ptr(self.tris), B, self.V, self.T,
                                                   _lib.ptr(keys), _lib.ptr(ids), _lib.current_stream()), "mesh_select")
        return ids

    def blend(self, screen, colours, ids):
        return _Blend.apply(self, screen, colours, ids)

    def __call__(self, rott_geo, texture, light, return_ids=False):
        colours = self.vertex_stage(rott_geo, texture, light)
        screen = self.screen(rott_geo)
        ids = self.select(screen)
        out = self.blend(screen, colours, ids)
        return (out, ids) if return_ids else out


# ---- the two fits ------------------------------------------------------------------------------------------------------
def light_frames(F, batch=32):
    """The frames of the light fit: arange(0, F, int(F / batch))[:batch] (face_tracker.py:215)."""
    if F < batch:
        raise ValueError(f"the photometric stages need at least {batch} frames, got {F}")
    return np.arange(0, F, int(F / batch))[:batch]


def fine_batches(F, batch=32):
    """[(start_n, end)] of the fine fit (face_tracker.py:290-297): the last batch is [F - batch, F)."""
    if F < batch:
        raise ValueError(f"the photometric stages need at least {batch} frames, got {F}")
    out = []
    for i in range(int((F - 1) / batch + 1)):
        out.append((F - batch, F) if (i + 1) * batch > F else (i * batch, i * batch + batch))
    return out


def light_schedule(iters=71):
    """Per iteration (lr factor, w_lan, w_regid, w_regexp): both rates are multiplied by 0.2 after the step of iteration 50
    (iter % 50 == 0 and iter > 0), the weights switch from iteration 51 (face_tracker.py:260-276)."""
    out, f = [], 1.0
    for it in range(iters):
        out.append((f,) + ((0.05, 1.0, 0.8) if it > 50 else (3.0, 2.0, 1.0)))
        if it % 50 == 0 and it > 0:
            f = f * 0.2
    return out


def fine_schedule(iters=50):
    """Per iteration w_lan: 8, and 1.5 from iteration 31 (face_tracker.py:379-382)."""
    return [1.5 if it > 30 else 8.0 for it in range(iters)]


def _check_mask(mask, frames):
    empty = (mask.flatten(1).sum(dim=1) == 0).nonzero().flatten().tolist()
    if empty:
        raise ValueError(f"frame {int(frames[empty[0]])}: the rendered mesh covers no pixel (the colour loss would be 0/0)")


def _load_images(images, frames, device, dtype):
    """images: a callable frames -> uint8 [n,H,W,3], or such an array / tensor over all frames."""
    got = images(list(int(f) for f in frames)) if callable(images) else images[torch.as_tensor(np.asarray(frames))]
    return torch.as_tensor(got).to(device=device, dtype=dtype)


def _fit_light(model, render, params, lms, images, focal, H, W, batch, iters, trace):
    dev, dtype = params["exp"].device, params["exp"].dtype
    F = int(params["exp"].shape[0])
    sel = light_frames(F, batch)
    sel_t = torch.as_tensor(sel, device=dev)
    imgs = _load_images(images, sel, dev, dtype)
    sel_lms = lms[sel_t]
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    tex = torch.zeros(1, model.tex_dim, dtype=dtype, device=dev, requires_grad=True)
    light = torch.zeros(batch, 27, dtype=dtype, device=dev, requires_grad=True)
    id_para = leaf(params["id"])
    # The reference hands Adam the whole [F,.] exp / euler / trans tensors.  Rows that are not selected get a zero
    # gradient, so their moments stay zero and Adam's update of them is 0 / (0 + eps) = 0: optimising the selected rows
    # alone is the same arithmetic.
    exp, euler, trans = leaf(params["exp"][sel_t]), leaf(params["euler"][sel_t]), leaf(params["trans"][sel_t])
    opt_tl = torch.optim.Adam([tex, light], lr=0.1)
    opt_idf = torch.optim.Adam([euler, trans, exp, id_para], lr=0.01)
    cx, cy = W / 2.0, H / 2.0
    for it, (f, w_lan, w_id, w_exp) in enumerate(light_schedule(iters)):
        for opt, lr in ((opt_tl, 0.1), (opt_idf, 0.01)):
            for g in opt.param_groups:
                g["lr"] = lr * f
        ids = id_para.expand(batch, -1)
        lands = landmarks_torch(model, ids, exp, euler, trans, focal, cx, cy)
        proj = project_torch(lands, euler, trans, focal, cx, cy)[:, :, :2]
        lan = torch.mean((proj - sel_lms) ** 2)
        reg_id, reg_exp = torch.mean(id_para * id_para), torch.mean(exp * exp)
        texture = texture_torch(model, tex.expand(batch, -1))
        rott = rott_torch(geometry_torch(model, ids, exp), euler, trans)
        img = render(rott, texture, light)
        mask = img[..., 3].detach() > 0.0
        if it == 0:
            _check_mask(mask, sel)
        col = color_loss_torch(img[..., :3], imgs, mask)
        loss = col + lan * w_lan + reg_id * w_id + reg_exp * w_exp
        opt_tl.zero_grad()
        opt_idf.zero_grad()
        loss.backward()
        opt_tl.step()
        opt_idf.step()
        if trace is not None:
            trace.append(dict(stage="light", iter=it, lr_tl=0.1 * f, lr_idf=0.01 * f, w_lan=w_lan, w_id=w_id, w_exp=w_exp,
                              col=float(col.detach()), lan=float(lan.detach()), frames=sel.tolist()))
    out = {k: v.detach().clone() for k, v in params.items()}
    out["id"] = id_para.detach()
    out["exp"][sel_t], out["euler"][sel_t], out["trans"][sel_t] = exp.detach(), euler.detach(), trans.detach()
    out["tex"] = tex.detach()
    out["light"] = light.detach().mean(dim=0, keepdim=True).repeat(F, 1)     # the mean light becomes every frame's
    return out


def _fit_frames(model, render, params, lms, images, focal, H, W, batch, iters, trace, pre_num=5):
    dev, dtype = params["exp"].device, params["exp"].dtype
    F = int(params["exp"].shape[0])
    if model.rigid_ids is None:
        raise ValueError("the fine fit needs rigid_ids (keys_info.npy)")
    out = {k: v.detach().clone() for k, v in params.items()}
    id_b = out["id"].expand(batch, -1)
    texture = texture_torch(model, out["tex"].expand(batch, -1))
    cx, cy = W / 2.0, H / 2.0
    for i, (a, b) in enumerate(fine_batches(F, batch)):
        frames = np.arange(a, b)
        imgs = _load_images(images, frames, dev, dtype)
        leaf = lambda t: t[a:b].detach().clone().requires_grad_(True)
        exp, euler, trans, light = leaf(out["exp"]), leaf(out["euler"]), leaf(out["trans"]), leaf(out["light"])
        opt = torch.optim.Adam([exp, euler, trans, light], lr=0.005)
        # the five frames before start_n, detached (fewer where a batch smaller than five leaves fewer in front of it)
        pre = slice(max(0, a - pre_num), a) if i > 0 else None
        for it, w_lan in enumerate(fine_schedule(iters)):
            lands = landmarks_torch(model, id_b, exp, euler, trans, focal, cx, cy)
            proj = project_torch(lands, euler, trans, focal, cx, cy)[:, :, :2]
            lan = torch.mean((proj - lms[a:b]) ** 2)
            reg_exp = torch.mean(exp * exp)
            rott = rott_torch(geometry_torch(model, id_b, exp), euler, trans)
            img = render(rott, texture, light)
            mask = img[..., 3].detach() > 0.0
            if it == 0:
                _check_mask(mask, frames)
            col = color_loss_torch(img[..., :3], imgs, mask)
            if pre is not None:
                e, r, t = (torch.cat((out[k][pre].detach(), v)) for k, v in (("exp", exp), ("euler", euler), ("trans", trans)))
            else:
                e, r, t = exp, euler, trans
            geo_lap = geometry_sub_torch(model, out["id"].expand(e.shape[0], -1), e, model.rigid_ids)
            rott_lap = rott_torch(geo_lap, r, t)
            lap = lap_loss_torch(rott_lap.reshape(rott_lap.shape[0], -1).permute(1, 0))
            loss = col * 0.5 + lan * w_lan + lap * 100000 + reg_exp * 1.0
            opt.zero_grad()
            loss.backward()
            opt.step()
            if trace is not None:
                trace.append(dict(stage="fine", batch=i, start=a, end=b, iter=it, w_lan=w_lan, col=float(col.detach()),
                                  lan=float(lan.detach()), lap=float(lap.detach()), lap_frames=int(e.shape[0])))
        out["exp"][a:b], out["euler"][a:b], out["trans"][a:b], out["light"][a:b] = \
            exp.detach(), euler.detach(), trans.detach(), light.detach()
    return out


def _statement_render(model, focal, H, W, device, settings):
    tris, vert_tris = model.topology_tensors(device)
    return lambda rott, texture, light: render_torch(rott, texture, light, tris, vert_tris, focal, H, W, **settings)


def _on(params, device, dtype):
    return {k: torch.as_tensor(v).to(device=device, dtype=dtype) for k, v in params.items() if k != "focal"}


def fit_light_torch(model, params, lms, images, focal, H, W, batch=32, iters=71, device="cpu", dtype=torch.float32, trace=None,
                    **settings):
    """The light fit (face_tracker.py:209-286) on the plain statement.  params: {"id" [1,I], "exp" [F,E], "euler" [F,3],
    "trans" [F,3]}; lms [F,68,2]; images: uint8 [F,H,W,3] or a callable frames -> uint8 [n,H,W,3].  -> params plus "tex"
    [1,tex_dim] and "light" [F,27].  ``settings``: sigma, gamma, blur_radius, ... of render_torch."""
    p = _on(params, device, dtype)
    lms = torch.as_tensor(lms).to(device=device, dtype=dtype)
    return _fit_light(model, _statement_render(model, focal, H, W, device, settings), p, lms, images, focal, H, W, batch, iters, trace)


def fit_frames_torch(model, params, lms, images, focal, H, W, batch=32, iters=50, device="cpu", dtype=torch.float32, trace=None,
                     **settings):
    """The frame-wise fine fit (face_tracker.py:288-406) on the plain statement; params as fit_light_torch returns them."""
    p = _on(params, device, dtype)
    lms = torch.as_tensor(lms).to(device=device, dtype=dtype)
    return _fit_frames(model, _statement_render(model, focal, H, W, device, settings), p, lms, images, focal, H, W, batch, iters, trace)


class PhotometricTracker:
    """The two fits on a HIP device: the loops of fit_light_torch / fit_frames_torch over MeshRenderer.  The landmark and
    regulariser terms are landmarks_torch / project_torch under autograd, the full-mesh geometry is torch.mm, the
    optimizer torch.optim.Adam; only the renderer is HIP."""

    def __init__(self, model: Face3DMM, device="cuda"):
        self.model, self.device = model, torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("PhotometricTracker runs on a HIP device; fit_light_torch / fit_frames_torch serve any other")
        if not (model.has_texture and model.has_topology):
            raise ValueError("the photometric stages need a Face3DMM with texture and topology")

    def _prepare(self, params, lms, focal, H, W, settings):
        p = _on(params, self.device, torch.float32)
        lms = torch.as_tensor(lms).to(device=self.device, dtype=torch.float32)
        return p, lms, MeshRenderer(self.model, focal, H, W, self.device, **settings)

    def fit_light(self, params, lms, images, focal, H, W, batch=32, iters=71, trace=None, **settings):
        p, lms, r = self._prepare(params, lms, focal, H, W, settings)
        return _fit_light(self.model, r, p, lms, images, focal, H, W, batch, iters, trace)

    def fit_frames(self, params, lms, images, focal, H, W, batch=32, iters=50, trace=None, **settings):
        p, lms, r = self._prepare(params, lms, focal, H, W, settings)
        return _fit_frames(self.model, r, p, lms, images, focal, H, W, batch, iters, trace)


def jpg_loader(ori_imgs_dir, frame_ids):
    """-> a callable frames -> uint8 [n,H,W,3]: ``ori_imgs/<id>.jpg`` decoded by PIL to RGB.  Raises if one is missing."""
    missing = [i for i in frame_ids if not os.path.exists(os.path.join(ori_imgs_dir, f"{i}.jpg"))]
    if missing:
        raise ValueError(f"the photometric stages need ori_imgs/<i>.jpg of every tracked frame; missing: {missing[:5]}"
                         f"{' ...' if len(missing) > 5 else ''}")

    def load(frames):
        from PIL import Image
        out = []
        for f in frames:
            with Image.open(os.path.join(ori_imgs_dir, f"{frame_ids[f]}.jpg")) as im:
                out.append(np.asarray(im.convert("RGB"), dtype=np.uint8))
        return torch.from_numpy(np.stack(out))
    return load


def refine(model, params, lms, images, H, W, device, batch=32, light_iters=71, fine_iters=50, **settings):
    """The two photometric stages after the coarse fit -> params with refined exp / euler / trans (and id): a CUDA device
    runs PhotometricTracker, any other the statements."""
    if not (model.has_texture and model.has_topology) or model.rigid_ids is None:
        raise ValueError("photometric=True needs a Face3DMM with texture (b_tex, mu_tex, sig_tex), rigid_ids and topology "
                         "(topology_info.npy)")
    focal = float(torch.as_tensor(params["focal"]).reshape(-1)[0])
    F = int(params["exp"].shape[0])
    if F < batch:
        raise ValueError(f"the photometric stages need at least {batch} frames, got {F}")
    device = torch.device(device)
    if device.type == "cuda":
        t = PhotometricTracker(model, device)
        p = t.fit_light(params, lms, images, focal, H, W, batch, light_iters, **settings)
        p = t.fit_frames(p, lms, images, focal, H, W, batch, fine_iters, **settings)
    else:
        p = fit_light_torch(model, params, lms, images, focal, H, W, batch, light_iters, device, **settings)
        p = fit_frames_torch(model, p, lms, images, focal, H, W, batch, fine_iters, device, **settings)
    out = {k: p[k].detach().float().cpu().contiguous() for k in ("id", "exp", "euler", "trans")}
    out["focal"] = torch.tensor([focal], dtype=torch.float32)
    return out
