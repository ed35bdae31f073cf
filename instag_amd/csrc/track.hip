// Head-pose tracking from 68 landmarks: the landmark stages of the reference's 3DMM fit
// (data_utils/face_tracking/face_tracker.py:62-205) as four kernels.  instag_amd/track.py states the same in torch.
//
//   geometry_kernel   one workgroup per frame:  geo[f] = mu + coef[f] x basis,  coef = (id of the frame's group, exp[f]),
//                     the M = 68 + 16 P candidate points.
//   pose_kernel       one wave per frame.  With id / exp fixed the candidates are constants and a frame's pose gradient
//                     depends on that frame alone (the mean's 1 / (136 F_group) is a factor), so all n Adam iterations
//                     of a frame run inside one launch, the candidates in LDS, pose and moments in registers;
//                     finish_pose_kernel then writes loss[g] by group_kernel's tree and advances the counters.
//   joint_kernel      (kernel A) one workgroup per frame: geometry into LDS, wave 0 evaluates the frame, then thread k
//                     back-propagates the 68 selected points to coefficient k through the transposed basis, updates
//                     pose and exp in place and leaves the frame's d id in did[f].
//   group_kernel      (kernel B) one workgroup per group: sums did and the frame losses in a fixed order, updates id,
//                     writes loss[g] and advances the group's step counters.
//
// Lane mapping of a frame's evaluation (one wave64): lane l takes candidates l&3, (l&3)+4, ... of contour slot l>>2
// (16 slots x 4 lanes), the four lanes of a slot combine by two xor shuffles (ties: the smaller candidate index, i.e.
// the first, as torch.argmin / argmax); then lane l takes landmark l and lanes 0..3 also landmark 64 + l.  The six pose
// gradients and the loss sum are reduced by a xor butterfly: a fixed order, and every lane ends with the same bits.
// No atomics, no grid barrier: iterations of the joint loop are separated by launch boundaries.
//
// Step counters, beta^t and the learning rates live in state[G][8] (fp64) on the device, so the launches of a segment
// all carry the same arguments: {step, beta1^step, beta2^step} of the pose optimizer, the same of the id / exp
// optimizer, lr_pose, lr_idexp.
#include "common.hpp"
#include "device_math.hpp"

namespace instag {
namespace {

constexpr int TRACK_LMS = 68;
constexpr int TRACK_SLOTS = 16;          // 8 left (landmarks 0..7), 8 right (landmarks 9..16)
constexpr int TRACK_MAX_GROUPS = 16;
constexpr int TRACK_MAX_DIM = 128;
constexpr int TRACK_MAX_P = 64;
constexpr int JOINT_THREADS = 256;
constexpr int GROUP_THREADS = 512;
constexpr double BETA1 = 0.9, BETA2 = 0.999;
constexpr float ADAM_EPS = 1e-8f;

enum StateSlot { S_STEP_POSE = 0, S_B1_POSE, S_B2_POSE, S_STEP_IDEXP, S_B1_IDEXP, S_B2_IDEXP, S_LR_POSE, S_LR_IDEXP,
                 S_COUNT };

struct Groups {
  int32_t G;
  int32_t start[TRACK_MAX_GROUPS + 1];
  float focal[TRACK_MAX_GROUPS];
};

struct Dev {                      // what the kernels read of instag_track_args
  const float *basis, *basis_t, *mu, *lms;
  float *id, *exp, *pose, *m_pose, *v_pose, *m_exp, *v_exp, *m_id, *v_id;
  double* state;
  float *geo, *did, *frame_loss, *loss;
  int32_t* sel;
  float *g_id, *g_exp, *g_pose;
  int32_t F, I, E, P, M3;         // M3 = 3 M
  float cx, cy;
};

__device__ __forceinline__ int group_of(const Groups& gr, int f) {
  int g = 0;
  for (int i = 1; i < gr.G; ++i) g += (f >= gr.start[i]) ? 1 : 0;
  return g;
}

// Adam step sizes of step t = step + 1 as torch evaluates them: fp64 scalars, then fp32 arithmetic on the tensors
struct AdamStep {
  float step_size, inv_bc2_sqrt;
};
__device__ __forceinline__ AdamStep adam_step_of(double b1t, double b2t, double lr) {   // b?t: beta^t of THIS step
  AdamStep a;
  a.step_size = (float)(lr / (1.0 - b1t));
  a.inv_bc2_sqrt = (float)sqrt(1.0 - b2t);
  return a;
}
__device__ __forceinline__ void adam_update(float& p, float& m, float& v, float g, const AdamStep& a) {
  m = m + (g - m) * (float)(1.0 - BETA1);
  v = v * (float)BETA2 + g * g * (float)(1.0 - BETA2);
  const float denom = sqrtf(v) / a.inv_bc2_sqrt + ADAM_EPS;
  p = p - a.step_size * (m / denom);
}

// A frame's evaluation runs in fp64 on the fp32 parameters and candidates: 68 + 16 P transforms per iteration are nothing
// next to the geometry, and the sequential rotations, the projection's division and the residual cancellation then add
// no rounding of their own to the gradients (measured against the fp64 statement: DESIGN section 20).
struct Rot {
  double ct, st, cp, sp, cs, ss;    // theta (x), phi (y), psi (z):  R = Rx Ry Rz
};
__device__ __forceinline__ Rot make_rot(double theta, double phi, double psi) {
  Rot r;
  sincos(theta, &r.st, &r.ct);
  sincos(phi, &r.sp, &r.cp);
  sincos(psi, &r.ss, &r.cs);
  return r;
}

struct Fwd {
  double q1x, q1y, q1z, q2x, q2y, q2z, X, Y, Z;
};
__device__ __forceinline__ Fwd transform(const Rot& r, double x, double y, double z, double tx, double ty, double tz) {
  Fwd w;
  w.q1x = r.cs * x + r.ss * y;   w.q1y = -r.ss * x + r.cs * y;   w.q1z = z;                     // Rz
  w.q2x = r.cp * w.q1x + r.sp * w.q1z;   w.q2y = w.q1y;   w.q2z = -r.sp * w.q1x + r.cp * w.q1z;  // Ry
  w.X = w.q2x + tx;                                                                              // Rx, + t
  w.Y = r.ct * w.q2y - r.st * w.q2z + ty;
  w.Z = r.st * w.q2y + r.ct * w.q2z + tz;
  return w;
}
__device__ __forceinline__ double project_x(const Fwd& w, double focal, double cx) { return -(focal * w.X) / w.Z + cx; }
__device__ __forceinline__ double project_y(const Fwd& w, double focal, double cy) { return (focal * w.Y) / w.Z + cy; }

// One wave evaluates one frame on the candidates geo[M][3] (LDS).  pose: theta, phi, psi, tx, ty, tz.  lm0 / lm1: the
// lane's landmark l and (lanes 0..3) 64 + l.  scale = 1 / (136 F_group).  Returns on every lane the seven sums
// {d theta, d phi, d psi, d tx, d ty, d tz, sum of squared residuals}.  gp != nullptr: also d loss / d (model point) of
// the 68 landmarks into gp[68][3] and the chosen point per landmark into pt[68] (LDS).  best_out: the lane's slot choice.
__device__ __forceinline__ void eval_frame(const float* geo, int P, const float pose[6], float focal_f, float cx_f,
                                           float cy_f, float2 lm0, float2 lm1, double scale, float out[7], float* gp,
                                           int* pt, int& best_out) {
  const int lane = threadIdx.x & 63;
  const Rot r = make_rot(pose[0], pose[1], pose[2]);
  const double tx = pose[3], ty = pose[4], tz = pose[5], focal = focal_f, cx = cx_f, cy = cy_f;

  // contour slots: left ones (0..7) take the smallest projected x, right ones (8..15) the largest
  const int slot = lane >> 2, sub = lane & 3;
  const double sign = slot < 8 ? 1.0 : -1.0;
  double bx = INFINITY;
  int bp = 0x7fffffff;
  for (int p = sub; p < P; p += 4) {
    const float* c = geo + (TRACK_LMS + slot * P + p) * 3;
    const Fwd w = transform(r, c[0], c[1], c[2], tx, ty, tz);
    const double x = sign * project_x(w, focal, cx);
    if (x < bx || bp == 0x7fffffff) { bx = x; bp = p; }      // ascending p: a later equal one never replaces
  }
#pragma unroll
  for (int m = 1; m <= 2; m <<= 1) {
    const double ox = __shfl_xor(bx, m, 64);
    const int op = __shfl_xor(bp, m, 64);
    if (op != 0x7fffffff && (bp == 0x7fffffff || ox < bx || (ox == bx && op < bp))) { bx = ox; bp = op; }
  }
  best_out = bp;

  double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int j = pass * 64 + lane;
    const int js = j < TRACK_LMS ? j : 0;
    const int sl = js < 8 ? js : js - 1;                       // landmarks 9..16 -> slots 8..15
    const bool contour = js < 8 || (js >= 9 && js < 17);
    const int chosen = __shfl(bp, (contour ? sl : 0) * 4, 64);
    if (pass == 1 && lane >= TRACK_LMS - 64) continue;          // (uniform shuffles are done)
    const int point = contour ? TRACK_LMS + sl * P + chosen : js;
    const float2 lm = pass == 0 ? lm0 : lm1;
    const float* c = geo + point * 3;
    const double x = c[0], y = c[1], z = c[2];
    const Fwd w = transform(r, x, y, z, tx, ty, tz);
    const double rx = project_x(w, focal, cx) - (double)lm.x, ry = project_y(w, focal, cy) - (double)lm.y;
    acc[6] += rx * rx + ry * ry;
    const double dx = 2.0 * scale * rx, dy = 2.0 * scale * ry;
    const double iz = 1.0 / w.Z;
    const double gX = -dx * focal * iz, gY = dy * focal * iz;
    const double gZ = (dx * focal * w.X - dy * focal * w.Y) * iz * iz;
    acc[3] += gX; acc[4] += gY; acc[5] += gZ;
    // back through Rx, Ry, Rz
    acc[0] += gY * (-r.st * w.q2y - r.ct * w.q2z) + gZ * (r.ct * w.q2y - r.st * w.q2z);
    const double h2x = gX, h2y = r.ct * gY + r.st * gZ, h2z = -r.st * gY + r.ct * gZ;
    acc[1] += h2x * (-r.sp * w.q1x + r.cp * w.q1z) + h2z * (-r.cp * w.q1x - r.sp * w.q1z);
    const double h1x = r.cp * h2x - r.sp * h2z, h1y = h2y, h1z = r.sp * h2x + r.cp * h2z;
    acc[2] += h1x * (-r.ss * x + r.cs * y) + h1y * (-r.cs * x - r.ss * y);
    if (gp) {
      gp[j * 3 + 0] = (float)(r.cs * h1x - r.ss * h1y);
      gp[j * 3 + 1] = (float)(r.ss * h1x + r.cs * h1y);
      gp[j * 3 + 2] = (float)h1z;
      pt[j] = point;
    }
  }
#pragma unroll
  for (int i = 0; i < 7; ++i) out[i] = (float)wave_sum(acc[i]);
}

__device__ __forceinline__ void lane_landmarks(const float* lms, int f, float2& lm0, float2& lm1) {
  const int lane = threadIdx.x & 63;
  const float2* l = reinterpret_cast<const float2*>(lms) + (size_t)f * TRACK_LMS;
  lm0 = l[lane];
  lm1 = lane < TRACK_LMS - 64 ? l[64 + lane] : make_float2(0.f, 0.f);
}

// geo[col] = mu[col] + sum_k coef[k] basis[k][col] for the block's columns; coef in LDS.  The K products are exact in
// fp64 and summed there (four chains), so a candidate carries one fp32 rounding instead of a K-term chain's.
__device__ __forceinline__ void geometry_columns(const Dev& d, const float* coef, float* dst) {
  const int K = d.I + d.E;
  for (int col = threadIdx.x; col < d.M3; col += blockDim.x) {
    const float* b = d.basis + col;
    double a0 = d.mu[col], a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int k = 0;
    for (; k + 4 <= K; k += 4) {
      a0 += (double)coef[k] * (double)b[(size_t)k * d.M3];
      a1 += (double)coef[k + 1] * (double)b[(size_t)(k + 1) * d.M3];
      a2 += (double)coef[k + 2] * (double)b[(size_t)(k + 2) * d.M3];
      a3 += (double)coef[k + 3] * (double)b[(size_t)(k + 3) * d.M3];
    }
    for (; k < K; ++k) a0 += (double)coef[k] * (double)b[(size_t)k * d.M3];
    dst[col] = (float)((a0 + a1) + (a2 + a3));
  }
}

__device__ __forceinline__ void load_coef(const Dev& d, int g, int f, float* coef) {
  for (int k = threadIdx.x; k < d.I + d.E; k += blockDim.x)
    coef[k] = k < d.I ? d.id[(size_t)g * d.I + k] : d.exp[(size_t)f * d.E + (k - d.I)];
}

__global__ void __launch_bounds__(JOINT_THREADS) track_geometry_kernel(Dev d, Groups gr) {
  __shared__ float coef[2 * TRACK_MAX_DIM];
  const int f = blockIdx.x;
  load_coef(d, group_of(gr, f), f, coef);
  __syncthreads();
  geometry_columns(d, coef, d.geo + (size_t)f * d.M3);
}

__global__ void track_set_lr_kernel(double* state, int G, double lr_pose, double lr_idexp) {
  const int g = threadIdx.x;
  if (g < G) {
    state[g * S_COUNT + S_LR_POSE] = lr_pose;
    state[g * S_COUNT + S_LR_IDEXP] = lr_idexp;
  }
}

// loss_lan of group g from the frames' sums: per thread frames tid, tid + 512, ..., then a tree over the threads (fp64)
__device__ __forceinline__ void group_loss(const Dev& d, int g, int f0, int f1, double* lsum) {
  const int tid = threadIdx.x;
  double l = 0.0;
  for (int f = f0 + tid; f < f1; f += GROUP_THREADS) l += (double)d.frame_loss[f];
  lsum[tid] = l;
  __syncthreads();
  for (int w = GROUP_THREADS / 2; w >= 1; w >>= 1) {
    if (tid < w) lsum[tid] += lsum[tid + w];
    __syncthreads();
  }
  if (tid == 0) d.loss[g] = (float)(lsum[0] / (double)(2 * TRACK_LMS * (f1 - f0)));
}

// after track_pose_kernel, one workgroup per group: loss[g] of the last iteration by group_kernel's tree, and the pose
// optimizer's counters after the n steps (the same products, in the same order)
__global__ void __launch_bounds__(GROUP_THREADS) track_finish_pose_kernel(Dev d, Groups gr, int n) {
  __shared__ double lsum[GROUP_THREADS];
  const int g = blockIdx.x;
  group_loss(d, g, gr.start[g], gr.start[g + 1], lsum);
  if (threadIdx.x != 0) return;
  double* s = d.state + g * S_COUNT;
  double b1 = s[S_B1_POSE], b2 = s[S_B2_POSE];
  for (int i = 0; i < n; ++i) { b1 *= BETA1; b2 *= BETA2; }
  s[S_B1_POSE] = b1; s[S_B2_POSE] = b2; s[S_STEP_POSE] += (double)n;
}

__global__ void __launch_bounds__(64) track_pose_kernel(Dev d, Groups gr, int n) {
  extern __shared__ float geo[];                       // [M][3]
  const int f = blockIdx.x, lane = threadIdx.x;
  const int g = group_of(gr, f);
  const float* src = d.geo + (size_t)f * d.M3;
  for (int i = lane; i < d.M3; i += 64) geo[i] = src[i];
  float2 lm0, lm1;
  lane_landmarks(d.lms, f, lm0, lm1);
  float pose[6], m[6], v[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    pose[i] = d.pose[(size_t)f * 6 + i];
    m[i] = d.m_pose[(size_t)f * 6 + i];
    v[i] = d.v_pose[(size_t)f * 6 + i];
  }
  const double* s = d.state + g * S_COUNT;
  double b1 = s[S_B1_POSE], b2 = s[S_B2_POSE];
  const double lr = s[S_LR_POSE];
  const float focal = gr.focal[g];
  const double scale = 1.0 / (double)(2 * TRACK_LMS * (gr.start[g + 1] - gr.start[g]));
  __syncthreads();
  float out[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int best = 0;
  for (int it = 0; it < n; ++it) {
    eval_frame(geo, d.P, pose, focal, d.cx, d.cy, lm0, lm1, scale, out, nullptr, nullptr, best);
    b1 *= BETA1; b2 *= BETA2;
    const AdamStep a = adam_step_of(b1, b2, lr);
#pragma unroll
    for (int i = 0; i < 6; ++i) adam_update(pose[i], m[i], v[i], out[i], a);
  }
  if (lane < 6) {                                       // (registers indexed by a constant per lane)
#pragma unroll
    for (int i = 0; i < 6; ++i)
      if (lane == i) {
        d.pose[(size_t)f * 6 + i] = pose[i];
        d.m_pose[(size_t)f * 6 + i] = m[i];
        d.v_pose[(size_t)f * 6 + i] = v[i];
      }
  }
  if (lane == 0 && n > 0) d.frame_loss[f] = out[6];
  if (d.sel && n > 0 && (lane & 3) == 0) d.sel[(size_t)f * TRACK_SLOTS + (lane >> 2)] = best;
}

// kernel A.  update = 0: instag_track_loss_grad (gradients out, nothing changed)
__global__ void __launch_bounds__(JOINT_THREADS) track_joint_kernel(Dev d, Groups gr, int update) {
  extern __shared__ float lds[];
  float* coef = lds;                                   // [256]
  float* gp = coef + 2 * TRACK_MAX_DIM;                // [68][3]
  int* pt = reinterpret_cast<int*>(gp + TRACK_LMS * 3);   // [68]
  float* geo = reinterpret_cast<float*>(pt + TRACK_LMS);  // [M][3]
  const int f = blockIdx.x, tid = threadIdx.x;
  const int g = group_of(gr, f);
  const int Fg = gr.start[g + 1] - gr.start[g];
  const double* s = d.state + g * S_COUNT;
  load_coef(d, g, f, coef);
  __syncthreads();
  geometry_columns(d, coef, geo);
  __syncthreads();

  if (tid < 64) {
    float2 lm0, lm1;
    lane_landmarks(d.lms, f, lm0, lm1);
    float pose[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) pose[i] = d.pose[(size_t)f * 6 + i];
    const double scale = 1.0 / (double)(2 * TRACK_LMS * Fg);
    float out[7];
    int best;
    eval_frame(geo, d.P, pose, gr.focal[g], d.cx, d.cy, lm0, lm1, scale, out, gp, pt, best);
    if (tid == 0) d.frame_loss[f] = out[6];
    if (d.sel && (tid & 3) == 0) d.sel[(size_t)f * TRACK_SLOTS + (tid >> 2)] = best;
    if (update) {
      const AdamStep a = adam_step_of(s[S_B1_POSE] * BETA1, s[S_B2_POSE] * BETA2, s[S_LR_POSE]);
#pragma unroll
      for (int i = 0; i < 6; ++i)
        if (tid == i) {
          float p = pose[i], m = d.m_pose[(size_t)f * 6 + i], v = d.v_pose[(size_t)f * 6 + i];
          adam_update(p, m, v, out[i], a);
          d.pose[(size_t)f * 6 + i] = p;
          d.m_pose[(size_t)f * 6 + i] = m;
          d.v_pose[(size_t)f * 6 + i] = v;
        }
    } else if (tid < 6) {
#pragma unroll
      for (int i = 0; i < 6; ++i)
        if (tid == i) d.g_pose[(size_t)f * 6 + i] = out[i];
    }
  }
  __syncthreads();

  // coefficient k: sum over the 68 chosen points, landmark order, x y z
  const int K = d.I + d.E;
  if (tid < K) {
    double sum = 0.0;
    for (int j = 0; j < TRACK_LMS; ++j) {
      const float* bt = d.basis_t + (size_t)pt[j] * 3 * K + tid;
      sum += (double)gp[j * 3 + 0] * (double)bt[0];
      sum += (double)gp[j * 3 + 1] * (double)bt[K];
      sum += (double)gp[j * 3 + 2] * (double)bt[2 * K];
    }
    float acc = (float)sum;
    if (tid < d.I) {
      d.did[(size_t)f * d.I + tid] = acc;
    } else {
      const int k = tid - d.I;
      const size_t o = (size_t)f * d.E + k;
      float p = coef[tid];
      acc = (float)(sum + 0.8 * (double)p / ((double)d.E * (double)Fg));   // 0.4 mean(exp^2) over the group's frames
      if (update) {
        const AdamStep a = adam_step_of(s[S_B1_IDEXP] * BETA1, s[S_B2_IDEXP] * BETA2, s[S_LR_IDEXP]);
        float m = d.m_exp[o], v = d.v_exp[o];
        adam_update(p, m, v, acc, a);
        d.exp[o] = p; d.m_exp[o] = m; d.v_exp[o] = v;
      } else {
        d.g_exp[o] = acc;
      }
    }
  }
}

// kernel B: thread (r, k) = (tid / 128, tid % 128) sums rows r, r + 4, ... of did[:, k] of the group, then the four
// partial sums are added in the order 0, 1, 2, 3; the frame losses likewise per thread, then a tree over the threads
__global__ void __launch_bounds__(GROUP_THREADS) track_group_kernel(Dev d, Groups gr, int update) {
  __shared__ double part[4][TRACK_MAX_DIM];
  __shared__ double lsum[GROUP_THREADS];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int f0 = gr.start[g], f1 = gr.start[g + 1];
  double* s = d.state + g * S_COUNT;
  const double b1 = s[S_B1_IDEXP] * BETA1, b2 = s[S_B2_IDEXP] * BETA2, lr = s[S_LR_IDEXP];
  const int r = tid >> 7, k = tid & 127;
  double acc = 0.0;
  if (k < d.I)
    for (int f = f0 + r; f < f1; f += 4) acc += (double)d.did[(size_t)f * d.I + k];
  part[r][k] = acc;
  group_loss(d, g, f0, f1, lsum);                     // (its barriers also publish part[][])
  if (tid < d.I) {
    const size_t o = (size_t)g * d.I + tid;
    float p = d.id[o];
    const float grad = (float)(((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid] + (double)p / (double)d.I);   // 0.5 mean(id^2)
    if (update) {
      const AdamStep a = adam_step_of(b1, b2, lr);
      float m = d.m_id[o], v = d.v_id[o];
      adam_update(p, m, v, grad, a);
      d.id[o] = p; d.m_id[o] = m; d.v_id[o] = v;
    } else {
      d.g_id[o] = grad;
    }
  }
  if (update && tid == 0) {          // every read of s in this block lies before the first barrier above
    s[S_B1_IDEXP] = b1; s[S_B2_IDEXP] = b2; s[S_STEP_IDEXP] += 1.0;
    s[S_B1_POSE] *= BETA1; s[S_B2_POSE] *= BETA2; s[S_STEP_POSE] += 1.0;
  }
}

size_t joint_lds_bytes(int M3) { return (size_t)(2 * TRACK_MAX_DIM + TRACK_LMS * 3 + TRACK_LMS + M3) * sizeof(float); }

enum Need { NEED_MOMENTS = 1, NEED_JOINT = 2, NEED_GRADS = 4 };

int check_args(const instag_track_args* a, int need, const char* what, Dev* d, Groups* gr) {
  const std::string w(what);
  INSTAG_REQUIRE(a != nullptr, w + ": NULL args");
  INSTAG_REQUIRE(a->basis && a->basis_t && a->mu && a->lms && a->id && a->exp && a->pose && a->state && a->geo &&
                 a->group_start && a->focal, w + ": NULL tensor");
  INSTAG_REQUIRE(a->frame_loss, w + ": NULL tensor");
  if (need & NEED_MOMENTS) INSTAG_REQUIRE(a->m_pose && a->v_pose, w + ": NULL tensor");
  if (need & NEED_JOINT) INSTAG_REQUIRE(a->did && a->loss, w + ": NULL tensor");
  if ((need & NEED_JOINT) && (need & NEED_MOMENTS))
    INSTAG_REQUIRE(a->m_exp && a->v_exp && a->m_id && a->v_id, w + ": NULL tensor");
  if (need & NEED_GRADS) INSTAG_REQUIRE(a->g_id && a->g_exp && a->g_pose, w + ": NULL tensor");
  INSTAG_REQUIRE(a->P >= 1 && a->P <= TRACK_MAX_P, w + ": P (candidates per contour slot) in 1 .. 64");
  INSTAG_REQUIRE(a->id_dim >= 1 && a->id_dim <= TRACK_MAX_DIM && a->exp_dim >= 1 && a->exp_dim <= TRACK_MAX_DIM,
                 w + ": id_dim and exp_dim in 1 .. 128");
  INSTAG_REQUIRE(a->n_landmarks == TRACK_LMS, w + ": 68 landmarks");
  INSTAG_REQUIRE(a->G >= 1 && a->G <= TRACK_MAX_GROUPS, w + ": 1 .. 16 groups");
  INSTAG_REQUIRE(a->group_start[0] == 0 && a->group_start[a->G] == a->F && a->F >= 1 && a->F <= (1 << 20),
                 w + ": groups must cover frames 0 .. F, F in 1 .. 2^20");
  for (int g = 0; g < a->G; ++g)
    INSTAG_REQUIRE(a->group_start[g + 1] > a->group_start[g], w + ": empty group");
  gr->G = a->G;
  for (int g = 0; g <= a->G; ++g) gr->start[g] = a->group_start[g];
  for (int g = 0; g < a->G; ++g) gr->focal[g] = a->focal[g];
  *d = Dev{a->basis, a->basis_t, a->mu, a->lms, a->id, a->exp, a->pose, a->m_pose, a->v_pose, a->m_exp, a->v_exp,
           a->m_id, a->v_id, a->state, a->geo, a->did, a->frame_loss, a->loss, a->sel, a->g_id, a->g_exp, a->g_pose,
           a->F, a->id_dim, a->exp_dim, a->P, 3 * (TRACK_LMS + TRACK_SLOTS * a->P), a->cx, a->cy};
  return INSTAG_OK;
}

}  // namespace
}  // namespace instag

using namespace instag;

extern "C" {

int instag_track_max_groups(void) { return TRACK_MAX_GROUPS; }

int instag_track_geometry(const instag_track_args* a, void* stream) {
  Dev d; Groups gr;
  if (int rc = check_args(a, 0, "track_geometry", &d, &gr)) return rc;
  track_geometry_kernel<<<d.F, JOINT_THREADS, 0, (hipStream_t)stream>>>(d, gr);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

int instag_track_fit_pose(const instag_track_args* a, int32_t n, double lr, void* stream) {
  Dev d; Groups gr;
  if (int rc = check_args(a, NEED_MOMENTS, "track_fit_pose", &d, &gr)) return rc;
  INSTAG_REQUIRE(a->loss != nullptr, "track_fit_pose: NULL tensor");
  INSTAG_REQUIRE(n >= 0, "track_fit_pose: n >= 0");
  if (n == 0) return INSTAG_OK;
  hipStream_t st = (hipStream_t)stream;
  track_set_lr_kernel<<<1, 64, 0, st>>>(d.state, gr.G, lr, lr);
  INSTAG_CHECK_LAUNCH();
  track_geometry_kernel<<<d.F, JOINT_THREADS, 0, st>>>(d, gr);
  INSTAG_CHECK_LAUNCH();
  track_pose_kernel<<<d.F, 64, (size_t)d.M3 * sizeof(float), st>>>(d, gr, n);
  INSTAG_CHECK_LAUNCH();
  track_finish_pose_kernel<<<gr.G, GROUP_THREADS, 0, st>>>(d, gr, n);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

int instag_track_fit_joint(const instag_track_args* a, int32_t n, double lr_pose, double lr_idexp, void* stream) {
  Dev d; Groups gr;
  if (int rc = check_args(a, NEED_MOMENTS | NEED_JOINT, "track_fit_joint", &d, &gr)) return rc;
  INSTAG_REQUIRE(n >= 0, "track_fit_joint: n >= 0");
  if (n == 0) return INSTAG_OK;
  hipStream_t st = (hipStream_t)stream;
  track_set_lr_kernel<<<1, 64, 0, st>>>(d.state, gr.G, lr_pose, lr_idexp);
  INSTAG_CHECK_LAUNCH();
  const size_t lds = joint_lds_bytes(d.M3);
  for (int it = 0; it < n; ++it) {
    track_joint_kernel<<<d.F, JOINT_THREADS, lds, st>>>(d, gr, 1);
    INSTAG_CHECK_LAUNCH();
    track_group_kernel<<<gr.G, GROUP_THREADS, 0, st>>>(d, gr, 1);
    INSTAG_CHECK_LAUNCH();
  }
  return INSTAG_OK;
}

int instag_track_loss_grad(const instag_track_args* a, void* stream) {
  Dev d; Groups gr;
  if (int rc = check_args(a, NEED_JOINT | NEED_GRADS, "track_loss_grad", &d, &gr)) return rc;
  hipStream_t st = (hipStream_t)stream;
  track_joint_kernel<<<d.F, JOINT_THREADS, joint_lds_bytes(d.M3), st>>>(d, gr, 0);
  INSTAG_CHECK_LAUNCH();
  track_group_kernel<<<gr.G, GROUP_THREADS, 0, st>>>(d, gr, 0);
  INSTAG_CHECK_LAUNCH();
  return INSTAG_OK;
}

}  // extern "C"
