// The 3DMM mesh renderer of the photometric tracking stages (instag_amd/mesh_render.py states what it computes).
//
//   vertex stage   one thread per (image, vertex): the unit normals of the vertex's M listed triangles are recomputed
//                  from the three corners (nothing per-triangle is stored), summed, normalised; nine SH values; colour =
//                  texture x lighting.  Backward: the same walk, gradients to texture (direct), to the light (a sum over
//                  V per image: wave shuffles, then the waves of a block, then the blocks, each in a fixed order) and to
//                  the corners of the listed triangles (float atomicAdd: a vertex collects from ~6 M threads).
//   selection      one thread per (image, triangle) walks the pixels of the triangle's bounding box grown by
//                  sqrt(blur_radius) / s and takes a 64-bit atomicMin on the key (float bits of pz) << 32 | face id; pz >= 0,
//                  so the bits order like the value and ties go to the lower face id.  A second pass takes the smallest
//                  key above the first.
//   blend          one thread per pixel recomputes barycentrics, distance and depth of its two faces from the ids.
//                  Backward: the same, then float atomicAdd into the screen vertices and the vertex colours.
//
// Every per-vertex and per-pixel evaluation runs in fp64 on the fp32 inputs: exp((zinv - zmax) / 1e-4) amplifies a depth
// rounding by 1e4, and the inside test, the clamps and the candidate test are decisions.  Results are stored as fp32.
#include "common.hpp"

namespace instag {
namespace {

constexpr int THREADS = 256;
constexpr double AREA_EPS = 1e-8;
constexpr double BARY_EPS = 1e-5;
constexpr double NORM_EPS = 1e-12;
constexpr int LIGHT = 27;

struct P3 { double x, y, z; };

struct Settings {
  int H, W;
  double s, sigma, gamma, blur, znear, zfar, eps, bg[3];
};

__host__ __device__ inline double sq(double a) { return a * a; }
__host__ __device__ inline double clamp01(double a) { return a < 0.0 ? 0.0 : (a > 1.0 ? 1.0 : a); }

__host__ __device__ inline double edge_fn(double px, double py, double ax, double ay, double bx, double by) {
  return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}

// squared distance of p to the segment a-b; a segment of squared length <= 1e-8 counts as its end point b
__host__ __device__ inline double seg_dist2(double px, double py, const P3& a, const P3& b) {
  const double dx = b.x - a.x, dy = b.y - a.y, l2 = dx * dx + dy * dy;
  if (l2 <= AREA_EPS) return sq(px - b.x) + sq(py - b.y);
  const double t = clamp01((dx * (px - a.x) + dy * (py - a.y)) / l2);
  // the end point itself at t = 1 (a + 0 d is a already): two edges whose nearest point is their shared corner tie exactly
  const double qx = t >= 1.0 ? b.x : a.x + t * dx, qy = t >= 1.0 ? b.y : a.y + t * dy;
  return sq(px - qx) + sq(py - qy);
}

// d/d(a, b) of g * seg_dist2.  Through an interior t nothing flows: the residual is perpendicular to the segment.
__host__ __device__ inline void seg_dist2_bwd(double px, double py, const P3& a, const P3& b, double g, P3& ga, P3& gb) {
  const double dx = b.x - a.x, dy = b.y - a.y, l2 = dx * dx + dy * dy;
  if (l2 <= AREA_EPS) {
    gb.x += -2.0 * (px - b.x) * g; gb.y += -2.0 * (py - b.y) * g;
    return;
  }
  const double t = clamp01((dx * (px - a.x) + dy * (py - a.y)) / l2);
  const double rx = px - (t >= 1.0 ? b.x : a.x + t * dx), ry = py - (t >= 1.0 ? b.y : a.y + t * dy);
  ga.x += -2.0 * rx * g * (1.0 - t); ga.y += -2.0 * ry * g * (1.0 - t);
  gb.x += -2.0 * rx * g * t;         gb.y += -2.0 * ry * g * t;
}

// d/d(a, b) of g * edge_fn(p; a, b)
__host__ __device__ inline void edge_bwd(double px, double py, const P3& a, const P3& b, double g, P3& ga, P3& gb) {
  ga.x += g * (py - b.y); ga.y += g * (b.x - px);
  gb.x += g * (a.y - py); gb.y += g * (px - a.x);
}

struct Face {
  double area, div, w[3], d[3], dist, sum, bc[3], pz;
  int e;
  bool inside, drawn;
};

__host__ __device__ inline void face_eval(double px, double py, const P3& a, const P3& b, const P3& c, Face& f) {
  f.area = edge_fn(c.x, c.y, a.x, a.y, b.x, b.y);
  f.drawn = fabs(f.area) > AREA_EPS;
  f.div = f.drawn ? f.area : 1.0;
  f.w[0] = edge_fn(px, py, b.x, b.y, c.x, c.y) / f.div;
  f.w[1] = edge_fn(px, py, c.x, c.y, a.x, a.y) / f.div;
  f.w[2] = edge_fn(px, py, a.x, a.y, b.x, b.y) / f.div;
  f.inside = f.w[0] > 0.0 && f.w[1] > 0.0 && f.w[2] > 0.0;
  f.d[0] = seg_dist2(px, py, a, b);
  f.d[1] = seg_dist2(px, py, b, c);
  f.d[2] = seg_dist2(px, py, c, a);
  f.e = 0;                                        // the first of equal distances
  double dmin = f.d[0];
  if (f.d[1] < dmin) { f.e = 1; dmin = f.d[1]; }
  if (f.d[2] < dmin) { f.e = 2; dmin = f.d[2]; }
  f.dist = f.inside ? -dmin : dmin;
  const double c0 = clamp01(f.w[0]), c1 = clamp01(f.w[1]), c2 = clamp01(f.w[2]);
  f.sum = c0 + c1 + c2;
  const double s = f.sum < BARY_EPS ? BARY_EPS : f.sum;
  f.bc[0] = c0 / s; f.bc[1] = c1 / s; f.bc[2] = c2 / s;
  f.pz = f.bc[0] * a.z + f.bc[1] * b.z + f.bc[2] * c.z;
}

// gradients of one face: g_bc = dL/d(clipped barycentrics) (without the depth term), g_pz, g_dist -> ga, gb, gc (x, y, z)
__host__ __device__ inline void face_bwd(double px, double py, const P3& a, const P3& b, const P3& c, const Face& f, double g_bc[3],
                                double g_pz, double g_dist, P3& ga, P3& gb, P3& gc) {
  ga.z += g_pz * f.bc[0]; gb.z += g_pz * f.bc[1]; gc.z += g_pz * f.bc[2];
  g_bc[0] += g_pz * a.z; g_bc[1] += g_pz * b.z; g_bc[2] += g_pz * c.z;
  const double s = f.sum < BARY_EPS ? BARY_EPS : f.sum;
  const double dot = f.sum >= BARY_EPS ? g_bc[0] * f.bc[0] + g_bc[1] * f.bc[1] + g_bc[2] * f.bc[2] : 0.0;
  double ge[3], g_area = 0.0;
  for (int i = 0; i < 3; ++i) {
    const double gw = (f.w[i] >= 0.0 && f.w[i] <= 1.0) ? (g_bc[i] - dot) / s : 0.0;
    ge[i] = gw / f.div;
    g_area -= gw * f.w[i] / f.div;
  }
  edge_bwd(px, py, b, c, ge[0], gb, gc);
  edge_bwd(px, py, c, a, ge[1], gc, ga);
  edge_bwd(px, py, a, b, ge[2], ga, gb);
  if (f.drawn) {
    edge_bwd(c.x, c.y, a, b, g_area, ga, gb);
    gc.x += g_area * (b.y - a.y); gc.y -= g_area * (b.x - a.x);
  }
  const double g_d = f.inside ? -g_dist : g_dist;
  if (f.e == 0) seg_dist2_bwd(px, py, a, b, g_d, ga, gb);
  else if (f.e == 1) seg_dist2_bwd(px, py, b, c, g_d, gb, gc);
  else seg_dist2_bwd(px, py, c, a, g_d, gc, ga);
}

// the three screen corners of face t of image b, x and y in units of s; false: an index outside the mesh
__host__ __device__ inline bool load_face(const float* __restrict__ screen, const int* __restrict__ tris, size_t b, int t, int V,
                                 double s, int idx[3], P3 p[3]) {
  for (int k = 0; k < 3; ++k) {
    idx[k] = tris[(size_t)t * 3 + k];
    if ((unsigned)idx[k] >= (unsigned)V) return false;
    const float* q = screen + (b * V + idx[k]) * 3;
    p[k].x = (double)q[0] * s; p[k].y = (double)q[1] * s; p[k].z = (double)q[2];
  }
  return true;
}

// ---- selection -----------------------------------------------------------------------------------------------------------
template <int PASS>
__global__ void __launch_bounds__(THREADS) mesh_select_kernel(Settings st, const float* __restrict__ screen,
                                                              const int* __restrict__ tris, int B, int V, int T,
                                                              unsigned long long* __restrict__ keys) {
  const size_t gid = (size_t)blockIdx.x * THREADS + threadIdx.x;
  if (gid >= (size_t)B * T) return;
  const size_t b = gid / T;
  const int t = (int)(gid % T);
  int idx[3]; P3 p[3];
  if (!load_face(screen, tris, b, t, V, st.s, idx, p)) return;
  for (int k = 0; k < 3; ++k)
    if (!(fabs(p[k].x) < 1e30) || !(fabs(p[k].y) < 1e30) || !(fabs(p[k].z) < 1e30)) return;    // inf / NaN: never a candidate
  const double area = edge_fn(p[2].x, p[2].y, p[0].x, p[0].y, p[1].x, p[1].y);
  if (!(fabs(area) > AREA_EPS)) return;
  if (!(fmax(fmax(p[0].z, p[1].z), p[2].z) >= 0.0)) return;
  // pixel centres (j + 0.5) s within the box grown by sqrt(blur_radius): floor / ceil leave up to a pixel of slack on
  // either side, far more than the roundings of these lines
  const double r = sqrt(fmax(st.blur, 0.0));
  double x0 = floor((fmin(fmin(p[0].x, p[1].x), p[2].x) - r) / st.s - 0.5);
  double x1 = ceil((fmax(fmax(p[0].x, p[1].x), p[2].x) + r) / st.s - 0.5);
  double y0 = floor((fmin(fmin(p[0].y, p[1].y), p[2].y) - r) / st.s - 0.5);
  double y1 = ceil((fmax(fmax(p[0].y, p[1].y), p[2].y) + r) / st.s - 0.5);
  if (x1 < 0.0 || y1 < 0.0 || x0 > st.W - 1 || y0 > st.H - 1) return;
  const int j0 = (int)fmax(x0, 0.0), j1 = (int)fmin(x1, (double)(st.W - 1));
  const int i0 = (int)fmax(y0, 0.0), i1 = (int)fmin(y1, (double)(st.H - 1));
  for (int i = i0; i <= i1; ++i) {
    const double py = (i + 0.5) * st.s;
    for (int j = j0; j <= j1; ++j) {
      const double px = (j + 0.5) * st.s;
      Face f;
      face_eval(px, py, p[0], p[1], p[2], f);
      if (!(f.pz >= 0.0) || !(f.inside || f.dist < st.blur)) continue;
      const unsigned long long key = ((unsigned long long)__float_as_uint(fabsf((float)f.pz)) << 32) | (unsigned)t;
      unsigned long long* slot = keys + ((b * st.H + i) * st.W + j) * 2;      // i < H, j < W by the clamps above
      // A slot only ever decreases, so a plain (possibly stale, hence larger) read can rule a key out: a pixel has a
      // dozen candidates and most of them arrive after a smaller one, which leaves the atomic to the few that may win.
      if (PASS == 0) {
        if (key < slot[0]) atomicMin(slot, key);
      } else if (key > slot[0] && key < slot[1]) {          // (slot[0] is final: the first pass has ended)
        atomicMin(slot + 1, key);
      }
    }
  }
}

__global__ void __launch_bounds__(THREADS) mesh_ids_kernel(const unsigned long long* __restrict__ keys, size_t n,
                                                           int* __restrict__ ids) {
  const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = keys[i];
  ids[i] = k == ~0ull ? -1 : (int)(unsigned)(k & 0xffffffffull);
}

// ---- blend ---------------------------------------------------------------------------------------------------------------
struct Slot {
  bool filled;
  int idx[3];
  P3 p[3];
  Face f;
  double prob, zinv, col[3], vcol[3][3];
};

__host__ __device__ inline void load_slot(const Settings& st, const float* __restrict__ screen, const float* __restrict__ colours,
                                 const int* __restrict__ tris, size_t b, int id, int V, int T, double px, double py, Slot& s) {
  s.filled = id >= 0 && id < T && load_face(screen, tris, b, id, V, st.s, s.idx, s.p);
  s.prob = 0.0; s.zinv = 0.0; s.col[0] = s.col[1] = s.col[2] = 0.0;
  if (!s.filled) return;
  face_eval(px, py, s.p[0], s.p[1], s.p[2], s.f);
  const double x = -s.f.dist / st.sigma;
  s.prob = x >= 0.0 ? 1.0 / (1.0 + exp(-x)) : exp(x) / (1.0 + exp(x));
  s.zinv = (st.zfar - s.f.pz) / (st.zfar - st.znear);
  for (int k = 0; k < 3; ++k) {
    const float* q = colours + (b * V + s.idx[k]) * 3;
    for (int c = 0; c < 3; ++c) s.vcol[k][c] = (double)q[c];
  }
  for (int c = 0; c < 3; ++c)
    s.col[c] = s.f.bc[0] * s.vcol[0][c] + s.f.bc[1] * s.vcol[1][c] + s.f.bc[2] * s.vcol[2][c];
}

struct Mix { double zraw, zmax, ex[2], wn[2], dexp, delta, den, rgb[3], alpha; };

__host__ __device__ inline void mix(const Settings& st, const Slot s[2], Mix& m) {
  m.zraw = fmax(s[0].zinv, s[1].zinv);
  m.zmax = fmax(m.zraw, st.eps);
  for (int k = 0; k < 2; ++k) {
    m.ex[k] = exp((s[k].zinv - m.zmax) / st.gamma);
    m.wn[k] = s[k].prob * m.ex[k];
  }
  m.dexp = exp((st.eps - m.zmax) / st.gamma);
  m.delta = fmax(m.dexp, st.eps);
  m.den = m.wn[0] + m.wn[1] + m.delta;
  for (int c = 0; c < 3; ++c) m.rgb[c] = (m.wn[0] * s[0].col[c] + m.wn[1] * s[1].col[c] + m.delta * st.bg[c]) / m.den;
  m.alpha = 1.0 - (1.0 - s[0].prob) * (1.0 - s[1].prob);
}

__host__ __device__ inline double clamp255(double a) { return a < 0.0 ? 0.0 : (a > 255.0 ? 255.0 : a); }

// the gradients one pixel sends to the corners of its two faces: colours [slot][corner][channel], screen (u, v, z)
struct PixelGrad { double col[2][3][3]; P3 vert[2][3]; };

__host__ __device__ inline void blend_pixel_bwd(const Settings& st, double px, double py, const Slot s[2], const Mix& m,
                                                const double gin[4], PixelGrad& pg) {
  // the output clamp passes a gradient inside [0, 255] (bounds included, as torch.clamp does)
  double g_num[3], g_den = 0.0;
  for (int c = 0; c < 3; ++c) {
    const double g = (m.rgb[c] >= 0.0 && m.rgb[c] <= 255.0) ? gin[c] : 0.0;
    g_num[c] = g / m.den;
    g_den -= g * m.rgb[c] / m.den;
  }
  const double g_alpha = (m.alpha >= 0.0 && m.alpha <= 255.0) ? gin[3] : 0.0;
  double g_delta = g_den, g_zmax = 0.0, g_zinv[2], g_prob[2];
  for (int c = 0; c < 3; ++c) g_delta += g_num[c] * st.bg[c];
  for (int k = 0; k < 2; ++k) {
    double g_wn = g_den;
    for (int c = 0; c < 3; ++c) g_wn += g_num[c] * s[k].col[c];
    g_prob[k] = g_wn * m.ex[k] + g_alpha * (1.0 - s[1 - k].prob);
    g_zinv[k] = g_wn * m.wn[k] / st.gamma;
    g_zmax -= g_zinv[k];
  }
  if (m.dexp >= st.eps) g_zmax -= g_delta * m.dexp / st.gamma;
  if (m.zraw >= st.eps) {
    if (s[0].zinv >= s[1].zinv) g_zinv[0] += g_zmax; else g_zinv[1] += g_zmax;
  }
  for (int k = 0; k < 2; ++k) {
    for (int v = 0; v < 3; ++v) {
      pg.vert[k][v] = P3{0.0, 0.0, 0.0};
      for (int c = 0; c < 3; ++c) pg.col[k][v][c] = 0.0;
    }
    if (!s[k].filled) continue;
    double g_bc[3] = {0.0, 0.0, 0.0};
    for (int v = 0; v < 3; ++v)
      for (int c = 0; c < 3; ++c) {
        g_bc[v] += g_num[c] * m.wn[k] * s[k].vcol[v][c];
        pg.col[k][v][c] = g_num[c] * m.wn[k] * s[k].f.bc[v];
      }
    const double g_pz = -g_zinv[k] / (st.zfar - st.znear);
    const double g_dist = -g_prob[k] * s[k].prob * (1.0 - s[k].prob) / st.sigma;
    face_bwd(px, py, s[k].p[0], s[k].p[1], s[k].p[2], s[k].f, g_bc, g_pz, g_dist, pg.vert[k][0], pg.vert[k][1], pg.vert[k][2]);
    for (int v = 0; v < 3; ++v) { pg.vert[k][v].x *= st.s; pg.vert[k][v].y *= st.s; }   // x, y were scaled by s on the way in
  }
}

__global__ void __launch_bounds__(THREADS) mesh_blend_forward_kernel(Settings st, const float* __restrict__ screen,
                                                                     const float* __restrict__ colours,
                                                                     const int* __restrict__ tris, const int* __restrict__ ids,
                                                                     int B, int V, int T, float* __restrict__ out) {
  const size_t pix = (size_t)blockIdx.x * THREADS + threadIdx.x;
  const size_t hw = (size_t)st.H * st.W;
  if (pix >= (size_t)B * hw) return;
  const size_t b = pix / hw;
  const int i = (int)((pix % hw) / st.W), j = (int)(pix % st.W);
  const int id0 = ids[pix * 2], id1 = ids[pix * 2 + 1];
  float4 o;
  if (id0 < 0 && id1 < 0) {                   // (rgb = delta bg / delta, alpha = 0)
    o = make_float4((float)clamp255(st.bg[0]), (float)clamp255(st.bg[1]), (float)clamp255(st.bg[2]), 0.f);
  } else {
    const double px = (j + 0.5) * st.s, py = (i + 0.5) * st.s;
    Slot s[2];
    load_slot(st, screen, colours, tris, b, id0, V, T, px, py, s[0]);
    load_slot(st, screen, colours, tris, b, id1, V, T, px, py, s[1]);
    Mix m;
    mix(st, s, m);
    o = make_float4((float)clamp255(m.rgb[0]), (float)clamp255(m.rgb[1]), (float)clamp255(m.rgb[2]), (float)clamp255(m.alpha));
  }
  reinterpret_cast<float4*>(out)[pix] = o;
}

__global__ void __launch_bounds__(THREADS) mesh_blend_backward_kernel(Settings st, const float* __restrict__ screen,
                                                                      const float* __restrict__ colours,
                                                                      const int* __restrict__ tris, const int* __restrict__ ids,
                                                                      const float* __restrict__ d_out, int B, int V, int T,
                                                                      float* __restrict__ d_screen, float* __restrict__ d_colours) {
  const size_t pix = (size_t)blockIdx.x * THREADS + threadIdx.x;
  const size_t hw = (size_t)st.H * st.W;
  if (pix >= (size_t)B * hw) return;
  const int id0 = ids[pix * 2], id1 = ids[pix * 2 + 1];
  if (id0 < 0 && id1 < 0) return;
  const float4 go = reinterpret_cast<const float4*>(d_out)[pix];
  if (go.x == 0.f && go.y == 0.f && go.z == 0.f && go.w == 0.f) return;
  const size_t b = pix / hw;
  const int i = (int)((pix % hw) / st.W), j = (int)(pix % st.W);
  const double px = (j + 0.5) * st.s, py = (i + 0.5) * st.s;
  Slot s[2];
  load_slot(st, screen, colours, tris, b, id0, V, T, px, py, s[0]);
  load_slot(st, screen, colours, tris, b, id1, V, T, px, py, s[1]);
  Mix m;
  mix(st, s, m);
  const double gin[4] = {(double)go.x, (double)go.y, (double)go.z, (double)go.w};
  PixelGrad pg;
  blend_pixel_bwd(st, px, py, s, m, gin, pg);
  for (int k = 0; k < 2; ++k) {
    if (!s[k].filled) continue;
    for (int v = 0; v < 3; ++v) {
      float* dc = d_colours + (b * V + s[k].idx[v]) * 3;
      float* ds = d_screen + (b * V + s[k].idx[v]) * 3;
      for (int c = 0; c < 3; ++c)
        if (pg.col[k][v][c] != 0.0) atomicAdd(dc + c, (float)pg.col[k][v][c]);
      if (pg.vert[k][v].x != 0.0) atomicAdd(ds + 0, (float)pg.vert[k][v].x);
      if (pg.vert[k][v].y != 0.0) atomicAdd(ds + 1, (float)pg.vert[k][v].y);
      if (pg.vert[k][v].z != 0.0) atomicAdd(ds + 2, (float)pg.vert[k][v].z);
    }
  }
}

// ---- vertex stage --------------------------------------------------------------------------------------------------------
constexpr double PI = 3.14159265358979323846;
struct ShConst { double y0, k1, k2; };
__host__ __device__ inline ShConst sh_const() {
  const double a0 = PI, a1 = 2.0 * PI / sqrt(3.0), a2 = 2.0 * PI / sqrt(8.0);
  const double c0 = 1.0 / sqrt(4.0 * PI), c1 = sqrt(3.0) / sqrt(4.0 * PI), c2 = 3.0 * sqrt(5.0) / sqrt(12.0 * PI);
  return ShConst{a0 * c0, a1 * c1, a2 * c2};
}
#define SH_D0 (0.5 / sqrt(3.0))

struct Tri { int idx[3]; double e1[3], e2[3], cr[3], len, u[3]; bool ok; };

__host__ __device__ inline void cross3(const double a[3], const double b[3], double o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

__host__ __device__ inline void tri_normal(const float* __restrict__ geo_b, const int* __restrict__ tris, int t, int V, Tri& r) {
  r.ok = true;
  double p[3][3];
  for (int k = 0; k < 3; ++k) {
    r.idx[k] = tris[(size_t)t * 3 + k];
    if ((unsigned)r.idx[k] >= (unsigned)V) { r.ok = false; r.u[0] = r.u[1] = r.u[2] = 0.0; return; }
    for (int c = 0; c < 3; ++c) p[k][c] = (double)geo_b[(size_t)r.idx[k] * 3 + c];
  }
  for (int c = 0; c < 3; ++c) { r.e1[c] = p[1][c] - p[0][c]; r.e2[c] = p[2][c] - p[0][c]; }
  cross3(r.e1, r.e2, r.cr);
  r.len = sqrt(r.cr[0] * r.cr[0] + r.cr[1] * r.cr[1] + r.cr[2] * r.cr[2]);
  const double d = r.len < NORM_EPS ? NORM_EPS : r.len;                  // F.normalize: x / max(|x|, 1e-12)
  for (int c = 0; c < 3; ++c) r.u[c] = r.cr[c] / d;
}

struct Vert { double vs[3], len, n[3], Y[9], lighting[3]; };

__host__ __device__ inline void vertex_eval(const float* __restrict__ geo_b, const int* __restrict__ tris,
                                   const int* __restrict__ vert_tris, const float* __restrict__ light_b, int v, int V, int T,
                                   int M, Vert& r) {
  r.vs[0] = r.vs[1] = r.vs[2] = 0.0;
  for (int m = 0; m < M; ++m) {
    const int t = vert_tris[(size_t)v * M + m];
    if ((unsigned)t >= (unsigned)T) continue;
    Tri tr;
    tri_normal(geo_b, tris, t, V, tr);
    for (int c = 0; c < 3; ++c) r.vs[c] += tr.u[c];
  }
  r.len = sqrt(r.vs[0] * r.vs[0] + r.vs[1] * r.vs[1] + r.vs[2] * r.vs[2]);
  for (int c = 0; c < 3; ++c) r.n[c] = r.vs[c] / r.len;
  const ShConst k = sh_const();
  const double nx = r.n[0], ny = r.n[1], nz = r.n[2];
  r.Y[0] = k.y0; r.Y[1] = -k.k1 * ny; r.Y[2] = k.k1 * nz; r.Y[3] = -k.k1 * nx; r.Y[4] = k.k2 * nx * ny;
  r.Y[5] = -k.k2 * ny * nz; r.Y[6] = k.k2 * SH_D0 * (3.0 * nz * nz - 1.0); r.Y[7] = -k.k2 * nx * nz;
  r.Y[8] = k.k2 * 0.5 * (nx * nx - ny * ny);
  for (int c = 0; c < 3; ++c) {
    double acc = 0.0;
    for (int q = 0; q < 9; ++q) acc += r.Y[q] * ((double)light_b[c * 9 + q] + (q == 0 ? 0.8 : 0.0));
    r.lighting[c] = acc;
  }
}

// one vertex's backward: dL/dcolour -> dL/dtexture, its 27 terms of dL/dlight, dL/d(sum of the listed unit normals)
__host__ __device__ inline void vertex_bwd(const Vert& r, const float* light_b, const double gcol[3], const double texv[3],
                                           double gtex[3], double g_light[27], double gvs[3]) {
  double gY[9];
  for (int q = 0; q < 9; ++q) gY[q] = 0.0;
  for (int c = 0; c < 3; ++c) {
    gtex[c] = gcol[c] * r.lighting[c];
    const double gl = gcol[c] * texv[c];
    for (int q = 0; q < 9; ++q) {
      g_light[c * 9 + q] = r.Y[q] * gl;
      gY[q] += ((double)light_b[c * 9 + q] + (q == 0 ? 0.8 : 0.0)) * gl;
    }
  }
  const ShConst k = sh_const();
  const double nx = r.n[0], ny = r.n[1], nz = r.n[2];
  double gn[3];
  gn[0] = -k.k1 * gY[3] + k.k2 * ny * gY[4] - k.k2 * nz * gY[7] + k.k2 * nx * gY[8];
  gn[1] = -k.k1 * gY[1] + k.k2 * nx * gY[4] - k.k2 * nz * gY[5] - k.k2 * ny * gY[8];
  gn[2] = k.k1 * gY[2] - k.k2 * ny * gY[5] + k.k2 * SH_D0 * 6.0 * nz * gY[6] - k.k2 * nx * gY[7];
  const double nd = nx * gn[0] + ny * gn[1] + nz * gn[2];
  for (int c = 0; c < 3; ++c) gvs[c] = (gn[c] - r.n[c] * nd) / r.len;
}

// dL/d(unit normal of a triangle) -> dL/d(its two edge vectors e1 = p1 - p0, e2 = p2 - p0)
__host__ __device__ inline void tri_bwd(const Tri& tr, const double gu[3], double ge1[3], double ge2[3]) {
  double gcr[3];
  if (tr.len >= NORM_EPS) {
    const double ud = tr.u[0] * gu[0] + tr.u[1] * gu[1] + tr.u[2] * gu[2];
    for (int c = 0; c < 3; ++c) gcr[c] = (gu[c] - tr.u[c] * ud) / tr.len;
  } else {
    for (int c = 0; c < 3; ++c) gcr[c] = gu[c] / NORM_EPS;
  }
  cross3(tr.e2, gcr, ge1);             // cr = e1 x e2: dL/de1 = e2 x g, dL/de2 = g x e1
  cross3(gcr, tr.e1, ge2);
}

__global__ void __launch_bounds__(THREADS) mesh_vertex_forward_kernel(const float* __restrict__ geo, const float* __restrict__ tex,
                                                                      const float* __restrict__ light, const int* __restrict__ tris,
                                                                      const int* __restrict__ vert_tris, int V, int T, int M,
                                                                      float* __restrict__ colours) {
  const int v = blockIdx.x * THREADS + threadIdx.x;
  const size_t b = blockIdx.y;
  if (v >= V) return;
  Vert r;
  vertex_eval(geo + b * V * 3, tris, vert_tris, light + b * LIGHT, v, V, T, M, r);
  const size_t o = (b * V + v) * 3;
  for (int c = 0; c < 3; ++c) colours[o + c] = (float)((double)tex[o + c] * r.lighting[c]);
}

// grid (blocks over V, B).  partial [B][gridDim.x][27] fp64: the block's sum of dL/dlight, always in the same order
__global__ void __launch_bounds__(THREADS) mesh_vertex_backward_kernel(const float* __restrict__ geo, const float* __restrict__ tex,
                                                                       const float* __restrict__ light, const int* __restrict__ tris,
                                                                       const int* __restrict__ vert_tris,
                                                                       const float* __restrict__ d_colours, int V, int T, int M,
                                                                       float* __restrict__ d_geo, float* __restrict__ d_tex,
                                                                       double* __restrict__ partial) {
  __shared__ double wave_sum[THREADS / 64][LIGHT];
  const int v = blockIdx.x * THREADS + threadIdx.x;
  const size_t b = blockIdx.y;
  const float* geo_b = geo + b * V * 3;
  const float* light_b = light + b * LIGHT;
  double g_light[LIGHT];
  for (int q = 0; q < LIGHT; ++q) g_light[q] = 0.0;
  if (v < V) {
    Vert r;
    vertex_eval(geo_b, tris, vert_tris, light_b, v, V, T, M, r);
    const size_t o = (b * V + v) * 3;
    double gcol[3], texv[3], gtex[3], gvs[3];
    for (int c = 0; c < 3; ++c) { gcol[c] = (double)d_colours[o + c]; texv[c] = (double)tex[o + c]; }
    vertex_bwd(r, light_b, gcol, texv, gtex, g_light, gvs);
    for (int c = 0; c < 3; ++c) d_tex[o + c] = (float)gtex[c];
    if (gvs[0] != 0.0 || gvs[1] != 0.0 || gvs[2] != 0.0) {
      for (int m = 0; m < M; ++m) {
        const int t = vert_tris[(size_t)v * M + m];
        if ((unsigned)t >= (unsigned)T) continue;
        Tri tr;
        tri_normal(geo_b, tris, t, V, tr);
        if (!tr.ok) continue;
        double ge1[3], ge2[3];
        tri_bwd(tr, gvs, ge1, ge2);
        float* g0 = d_geo + (b * V + tr.idx[0]) * 3;
        float* g1 = d_geo + (b * V + tr.idx[1]) * 3;
        float* g2 = d_geo + (b * V + tr.idx[2]) * 3;
        for (int c = 0; c < 3; ++c) {
          atomicAdd(g0 + c, (float)(-(ge1[c] + ge2[c])));
          atomicAdd(g1 + c, (float)ge1[c]);
          atomicAdd(g2 + c, (float)ge2[c]);
        }
      }
    }
  }
  // the light gradient: lanes of a wave (a fixed shuffle tree), then the block's waves in order
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int q = 0; q < LIGHT; ++q) {
    double x = g_light[q];
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    if (lane == 0) wave_sum[wave][q] = x;
  }
  __syncthreads();
  if (threadIdx.x < LIGHT) {
    double x = wave_sum[0][threadIdx.x];
    for (int w = 1; w < THREADS / 64; ++w) x += wave_sum[w][threadIdx.x];
    partial[(b * gridDim.x + blockIdx.x) * LIGHT + threadIdx.x] = x;
  }
}

__global__ void __launch_bounds__(64) mesh_light_finish_kernel(const double* __restrict__ partial, int blocks,
                                                               float* __restrict__ d_light) {
  const size_t b = blockIdx.x;
  if (threadIdx.x >= LIGHT) return;
  double x = 0.0;
  for (int i = 0; i < blocks; ++i) x += partial[(b * blocks + i) * LIGHT + threadIdx.x];
  d_light[b * LIGHT + threadIdx.x] = (float)x;
}

int check_settings(const instag_mesh_settings* s, const char* what, Settings* o) {
  const std::string w(what);
  INSTAG_REQUIRE(s != nullptr, w + ": NULL settings");
  INSTAG_REQUIRE(s->H >= 1 && s->W >= 2 && s->H <= 16384 && s->W <= 16384, w + ": H in 1 .. 16384, W in 2 .. 16384");
  INSTAG_REQUIRE(s->W % 2 == 0, w + ": the image width must be even");
  INSTAG_REQUIRE(s->K == 2, w + ": K = 2 faces per pixel");
  INSTAG_REQUIRE(s->sigma > 0.0 && s->gamma > 0.0 && s->blur_radius >= 0.0 && s->zfar > s->znear && s->eps > 0.0,
                 w + ": sigma, gamma, eps > 0, blur_radius >= 0, zfar > znear");
  *o = Settings{s->H, s->W, 2.0 / (double)std::min(s->H, s->W), s->sigma, s->gamma, s->blur_radius, s->znear, s->zfar, s->eps,
                {s->bg_r, s->bg_g, s->bg_b}};
  return INSTAG_OK;
}

int check_mesh(int B, int V, int T, const char* what) {
  const std::string w(what);
  INSTAG_REQUIRE(B >= 1 && B <= 65535 && V >= 3 && T >= 1 && V <= (1 << 24) && T <= (1 << 26), w + ": B in 1 .. 65535, V >= 3, T >= 1");
  return INSTAG_OK;
}

}  // namespace
}  // namespace instag

using namespace instag;

extern "C" {

int instag_mesh_vertex_forward(const float* rott_geo, const float* texture, const float* light, const int32_t* tris,
                               const int32_t* vert_tris, int32_t B, int32_t V, int32_t T, int32_t M, float* colours,
                               void* stream) {
  INSTAG_REQUIRE(rott_geo && texture && light && tris && vert_tris && colours, "mesh_vertex_forward: NULL tensor");
  if (int rc = check_mesh(B, V, T, "mesh_vertex_forward")) return rc;
  INSTAG_REQUIRE(M >= 1 && M <= 1024, "mesh_vertex_forward: M (triangles listed per vertex) in 1 .. 1024");
  mesh_vertex_forward_kernel<<<dim3(div_up(V, THREADS), B), THREADS, 0, (hipStream_t)stream>>>(rott_geo, texture, light, tris,
                                                                                              vert_tris, V, T, M, colours);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

size_t instag_mesh_vertex_backward_workspace_bytes(int32_t B, int32_t V) {
  if (B < 1 || V < 1) return 0;
  return (size_t)B * div_up(V, THREADS) * LIGHT * sizeof(double);
}

int instag_mesh_vertex_backward(const float* rott_geo, const float* texture, const float* light, const int32_t* tris,
                                const int32_t* vert_tris, const float* d_colours, int32_t B, int32_t V, int32_t T, int32_t M,
                                float* d_rott_geo, float* d_texture, float* d_light, void* workspace, size_t workspace_bytes,
                                void* stream) {
  INSTAG_REQUIRE(rott_geo && texture && light && tris && vert_tris && d_colours && d_rott_geo && d_texture && d_light && workspace,
                 "mesh_vertex_backward: NULL tensor");
  if (int rc = check_mesh(B, V, T, "mesh_vertex_backward")) return rc;
  INSTAG_REQUIRE(M >= 1 && M <= 1024, "mesh_vertex_backward: M (triangles listed per vertex) in 1 .. 1024");
  if (workspace_bytes < instag_mesh_vertex_backward_workspace_bytes(B, V)) {
    set_error("mesh_vertex_backward: workspace too small");
    return INSTAG_E_SPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int blocks = div_up(V, THREADS);
  INSTAG_CHECK_HIP(hipMemsetAsync(d_rott_geo, 0, (size_t)B * V * 3 * sizeof(float), st));
  mesh_vertex_backward_kernel<<<dim3(blocks, B), THREADS, 0, st>>>(rott_geo, texture, light, tris, vert_tris, d_colours, V, T, M,
                                                                   d_rott_geo, d_texture, (double*)workspace);
  INSTAG_CHECK_LAUNCH();
  mesh_light_finish_kernel<<<B, 64, 0, st>>>((const double*)workspace, blocks, d_light);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

int instag_mesh_select(const instag_mesh_settings* settings, const float* screen, const int32_t* tris, int32_t B, int32_t V,
                       int32_t T, void* keys, int32_t* ids, void* stream) {
  Settings s;
  if (int rc = check_settings(settings, "mesh_select", &s)) return rc;
  INSTAG_REQUIRE(screen && tris && keys && ids, "mesh_select: NULL tensor");
  if (int rc = check_mesh(B, V, T, "mesh_select")) return rc;
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)B * s.H * s.W * 2;
  INSTAG_REQUIRE(n / 2 <= ((size_t)1 << 31), "mesh_select: B H W up to 2^31 pixels");
  INSTAG_CHECK_HIP(hipMemsetAsync(keys, 0xff, n * sizeof(unsigned long long), st));
  const unsigned blocks = (unsigned)div_up((size_t)B * T, (size_t)THREADS);
  mesh_select_kernel<0><<<blocks, THREADS, 0, st>>>(s, screen, tris, B, V, T, (unsigned long long*)keys);
  INSTAG_CHECK_LAUNCH();
  mesh_select_kernel<1><<<blocks, THREADS, 0, st>>>(s, screen, tris, B, V, T, (unsigned long long*)keys);
  INSTAG_CHECK_LAUNCH();
  mesh_ids_kernel<<<(unsigned)div_up(n, (size_t)THREADS), THREADS, 0, st>>>((const unsigned long long*)keys, n, ids);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

int instag_mesh_blend_forward(const instag_mesh_settings* settings, const float* screen, const float* colours,
                              const int32_t* tris, const int32_t* ids, int32_t B, int32_t V, int32_t T, float* out,
                              void* stream) {
  Settings s;
  if (int rc = check_settings(settings, "mesh_blend_forward", &s)) return rc;
  INSTAG_REQUIRE(screen && colours && tris && ids && out, "mesh_blend_forward: NULL tensor");
  if (int rc = check_mesh(B, V, T, "mesh_blend_forward")) return rc;
  const size_t n = (size_t)B * s.H * s.W;
  INSTAG_REQUIRE(n <= ((size_t)1 << 31), "mesh_blend_forward: B H W up to 2^31 pixels");
  mesh_blend_forward_kernel<<<(unsigned)div_up(n, (size_t)THREADS), THREADS, 0, (hipStream_t)stream>>>(s, screen, colours, tris, ids,
                                                                                                      B, V, T, out);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

int instag_mesh_blend_backward(const instag_mesh_settings* settings, const float* screen, const float* colours,
                               const int32_t* tris, const int32_t* ids, const float* d_out, int32_t B, int32_t V, int32_t T,
                               float* d_screen, float* d_colours, void* stream) {
  Settings s;
  if (int rc = check_settings(settings, "mesh_blend_backward", &s)) return rc;
  INSTAG_REQUIRE(screen && colours && tris && ids && d_out && d_screen && d_colours, "mesh_blend_backward: NULL tensor");
  if (int rc = check_mesh(B, V, T, "mesh_blend_backward")) return rc;
  const size_t n = (size_t)B * s.H * s.W;
  INSTAG_REQUIRE(n <= ((size_t)1 << 31), "mesh_blend_backward: B H W up to 2^31 pixels");
  hipStream_t st = (hipStream_t)stream;
  INSTAG_CHECK_HIP(hipMemsetAsync(d_screen, 0, (size_t)B * V * 3 * sizeof(float), st));
  INSTAG_CHECK_HIP(hipMemsetAsync(d_colours, 0, (size_t)B * V * 3 * sizeof(float), st));
  mesh_blend_backward_kernel<<<(unsigned)div_up(n, (size_t)THREADS), THREADS, 0, st>>>(s, screen, colours, tris, ids, d_out, B, V, T,
                                                                                      d_screen, d_colours);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

}  // extern "C"
