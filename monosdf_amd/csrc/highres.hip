// Merge of overlapping monocular cue patches into one mosaic per image (ABI: include/monosdf_highres.h), the device
// half of utils/highres_cues.py.  A merge is a chain of dependent steps (fit a patch to the running mosaic over their
// overlap, cross-fade it in); the chain is laid out as launches on the caller's stream, three per step:
//   * hrc_reduce_k: one workgroup per (chain, tile of 2048 overlap elements) -> partial sums in fp64
//   * hrc_solve_k:  one wave per chain adds the partials in a fixed order, one lane solves (scale and shift, or the
//                   rotation by a one-sided Jacobi SVD) and writes the coefficients into the `steps` array
//   * hrc_apply_k:  one workgroup per (chain, tile of 2048 patch elements) reads the coefficients, transforms, blends
//                   and stores
// A chain is (image, row) in the row phase, where every step moves all rows of all images one patch to the right, and
// an image in the column phase.  No workgroup waits on another, nothing is atomic, nothing returns to the host.
// Every patch element is read once by the reduce (its overlap part) and once by the apply; every mosaic element is
// written once, the overlap read twice more (normals: the head of a chain's first patch is renormalised in place once).  The same three kernels serve depth (fp32 storage, 4 sums) and normals
// (fp64 storage, 3 channels, 9 sums) and both axes: a view gives the address of (chain, channel, line, cross), a
// line being a column in the row phase and a row in the column phase.
//
// Built with -ffp-contract=off: every product and sum is rounded on its own, as the header states and the float64
// restatement of the tests (tests/highres_numpy.py) computes.
#include "tool_common.h"
#include "rotation_solve.h"
#include "../../include/monosdf_highres.h"

namespace {

constexpr int HRC_THREADS = 256;                        // 4 waves
constexpr int HRC_WAVES = HRC_THREADS / MSDF_WAVE;
constexpr int HRC_EPT = 8;                              // elements per lane
constexpr int HRC_TILE = HRC_THREADS * HRC_EPT;         // elements per workgroup

template <int NCH> struct HrcCue;
template <> struct HrcCue<1> { typedef float T; static constexpr int NS = 4, K = 2; };
template <> struct HrcCue<3> { typedef double T; static constexpr int NS = 9, K = 9; };

// Where element (line, cross) of channel ch of chain (image n, part s) lives.  `alt`: where part 0 lives instead
// (row strip 0 is built in the output); `base` then holds the parts 1, 2, .. only.
template <typename T>
struct HrcView {
  T* base;
  T* alt;
  int64_t img, sub, ch, alt_img, alt_ch, line, cross, off;
  __device__ __forceinline__ T* chain(int n, int s, int64_t& chs) const {
    if (alt != nullptr && s == 0) {
      chs = alt_ch;
      return alt + (int64_t)n * alt_img + off;
    }
    chs = ch;
    return base + (int64_t)n * img + (int64_t)(s - (alt != nullptr ? 1 : 0)) * sub + off;
  }
};

// The index space of one launch: `lines` x `cross` elements per chain, cut into n_tiles tiles; `subs` chains per image.
struct HrcGeom {
  int subs, lines, cross, line_fast, n_tiles;
};

__device__ __forceinline__ void hrc_split(const HrcGeom& g, int e, int& i, int& j) {
  if (g.line_fast) {
    j = e / g.lines;
    i = e - j * g.lines;
  } else {
    i = e / g.cross;
    j = e - i * g.cross;
  }
}

// Where the coefficients of this launch's step are: steps[n][step0 + s * step_sub][K]
struct HrcStepRef {
  double* steps;
  int n_steps, step0, step_sub;
};

// ---------------------------------------------------------------- sums over the overlap

template <int NCH>
__global__ void __launch_bounds__(HRC_THREADS)
hrc_reduce_k(HrcView<typename HrcCue<NCH>::T> pv, HrcView<typename HrcCue<NCH>::T> tv, HrcGeom g,
             double* __restrict__ part) {
  typedef typename HrcCue<NCH>::T T;
  constexpr int NS = HrcCue<NCH>::NS;
  __shared__ double red[HRC_WAVES][NS];
  const int t = (int)threadIdx.x, lane = lane_id(), wave = t / MSDF_WAVE;
  const int chain = (int)(blockIdx.x / (unsigned)g.n_tiles), tile = (int)(blockIdx.x % (unsigned)g.n_tiles);
  const int n = chain / g.subs, s = chain - n * g.subs;
  int64_t pch, tch;
  const T* p = pv.chain(n, s, pch);
  const T* q = tv.chain(n, s, tch);
  const int total = g.lines * g.cross;

  double acc[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) acc[k] = 0.0;
#pragma unroll
  for (int k = 0; k < HRC_EPT; ++k) {
    const int e = tile * HRC_TILE + k * HRC_THREADS + t;
    if (e < total) {
      int i, j;
      hrc_split(g, e, i, j);
      const int64_t po = (int64_t)i * pv.line + (int64_t)j * pv.cross, to = (int64_t)i * tv.line + (int64_t)j * tv.cross;
      if constexpr (NCH == 1) {
        const double a = (double)p[po], b = (double)q[to];
        acc[0] += a * a;
        acc[1] += a;
        acc[2] += a * b;
        acc[3] += b;
      } else {
        double a[3], b[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          a[c] = p[po + c * pch];
          b[c] = q[to + c * tch];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
          for (int d = 0; d < 3; ++d) acc[3 * c + d] += a[c] * b[d];
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const double v = wave_sum(acc[k]);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (t < NS) part[(size_t)blockIdx.x * NS + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

// ---------------------------------------------------------------- the solves, on one lane

__device__ void hrc_solve_depth(const double* s, double count, double* out) {
  const double a00 = s[0], a01 = s[1], a11 = count, b0 = s[2], b1 = s[3];
  const double det = a00 * a11 - a01 * a01;
  double scale = 0.0, shift = 0.0;
  if (det != 0.0) {
    scale = (a11 * b0 - a01 * b1) / det;
    shift = (-a01 * b0 + a00 * b1) / det;
  }
  out[0] = scale;
  out[1] = shift;
}

template <int NCH>
__global__ void __launch_bounds__(MSDF_WAVE)
hrc_solve_k(const double* __restrict__ part, int n_tiles, int subs, double count, HrcStepRef ref) {
  constexpr int NS = HrcCue<NCH>::NS, K = HrcCue<NCH>::K;
  const int chain = (int)blockIdx.x, lane = lane_id();
  const int n = chain / subs, s = chain - n * subs;
  double acc[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) acc[k] = 0.0;
  for (int tile = lane; tile < n_tiles; tile += MSDF_WAVE) {
    const double* p = part + ((size_t)chain * n_tiles + tile) * NS;
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] += p[k];
  }
#pragma unroll
  for (int k = 0; k < NS; ++k) acc[k] = wave_sum(acc[k]);
  if (lane == 0) {
    double* out = ref.steps + ((size_t)n * ref.n_steps + ref.step0 + (size_t)s * ref.step_sub) * K;
    if constexpr (NCH == 1) {
      hrc_solve_depth(acc, count, out);
    } else {
      solve_rotation(acc, out);                          // rotation_solve.h
    }
  }
}

// ---------------------------------------------------------------- transform, blend, store

// qv: the patch, `g.lines` lines of which the first O overlap the mosaic; mv: the mosaic from its first overlap line.
// ref.steps == nullptr: a plain copy (the first patch of a row).
template <int NCH>
__global__ void __launch_bounds__(HRC_THREADS)
hrc_apply_k(HrcView<typename HrcCue<NCH>::T> qv, HrcView<typename HrcCue<NCH>::T> mv, HrcGeom g, int O, double wstep,
            HrcStepRef ref) {
  typedef typename HrcCue<NCH>::T T;
  constexpr int K = HrcCue<NCH>::K;
  const int t = (int)threadIdx.x;
  const int chain = (int)(blockIdx.x / (unsigned)g.n_tiles), tile = (int)(blockIdx.x % (unsigned)g.n_tiles);
  const int n = chain / g.subs, s = chain - n * g.subs;
  int64_t qch, mch;
  const T* q = qv.chain(n, s, qch);
  T* m = mv.chain(n, s, mch);
  const int total = g.lines * g.cross;
  const bool copy = ref.steps == nullptr;
  double c[K];
#pragma unroll
  for (int k = 0; k < K; ++k) c[k] = 0.0;
  if (!copy) {
    const double* src = ref.steps + ((size_t)n * ref.n_steps + ref.step0 + (size_t)s * ref.step_sub) * K;
#pragma unroll
    for (int k = 0; k < K; ++k) c[k] = src[k];
  }
#pragma unroll
  for (int k = 0; k < HRC_EPT; ++k) {
    const int e = tile * HRC_TILE + k * HRC_THREADS + t;
    if (e >= total) continue;
    int i, j;
    hrc_split(g, e, i, j);
    const int64_t qo = (int64_t)i * qv.line + (int64_t)j * qv.cross, mo = (int64_t)i * mv.line + (int64_t)j * mv.cross;
    if (copy) {
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) m[mo + ch * mch] = q[qo + ch * qch];
      continue;
    }
    const double w = i == O - 1 ? 0.0 : (double)i * wstep + 1.0;
    if constexpr (NCH == 1) {
      double v = c[0] * (double)q[qo] + c[1];
      if (i < O) v = (double)m[mo] * w + v * (1.0 - w);
      m[mo] = (float)v;
    } else {
      const double x = q[qo], y = q[qo + qch], z = q[qo + 2 * qch];
      double v[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) v[a] = (c[3 * a] * x + c[3 * a + 1] * y) + c[3 * a + 2] * z;
      if (i < O) {
#pragma unroll
        for (int a = 0; a < 3; ++a) v[a] = m[mo + a * mch] * w + v[a] * (1.0 - w);
      }
      const double len = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + 1e-15;
#pragma unroll
      for (int a = 0; a < 3; ++a) m[mo + a * mch] = v[a] / len;
    }
  }
}

// normals: the reference divides the WHOLE mosaic by its length at every step, which changes more than the last bit
// only the first time a pixel meets it (the decoded patches are unit vectors in fp32 only).  The pixels a step writes
// are divided by hrc_apply_k; the lines of a chain's first patch in front of its first overlap are divided here,
// during that first step.  The sums of that step read the overlap alone, which this kernel does not touch.
__global__ void __launch_bounds__(HRC_THREADS)
hrc_renorm_k(HrcView<double> mv, HrcGeom g) {
  const int chain = (int)(blockIdx.x / (unsigned)g.n_tiles), tile = (int)(blockIdx.x % (unsigned)g.n_tiles);
  const int n = chain / g.subs, s = chain - n * g.subs;
  int64_t mch;
  double* m = mv.chain(n, s, mch);
  const int total = g.lines * g.cross;
#pragma unroll
  for (int k = 0; k < HRC_EPT; ++k) {
    const int e = tile * HRC_TILE + k * HRC_THREADS + (int)threadIdx.x;
    if (e >= total) continue;
    int i, j;
    hrc_split(g, e, i, j);
    const int64_t mo = (int64_t)i * mv.line + (int64_t)j * mv.cross;
    const double x = m[mo], y = m[mo + mch], z = m[mo + 2 * mch];
    const double len = sqrt((x * x + y * y) + z * z) + 1e-15;
    m[mo] = x / len;
    m[mo + mch] = y / len;
    m[mo + 2 * mch] = z / len;
  }
}

// ---------------------------------------------------------------- the end of a merge

// depth: out = scale out + shift where a centre fit was made (ref.steps), and the minimum and maximum of the stored
// values per tile
__global__ void __launch_bounds__(HRC_THREADS)
hrc_depth_affine_k(float* __restrict__ out, int hw, int n_tiles, HrcStepRef ref, double* __restrict__ part) {
  __shared__ float red[HRC_WAVES][2];
  const int t = (int)threadIdx.x, lane = lane_id(), wave = t / MSDF_WAVE;
  const int n = (int)(blockIdx.x / (unsigned)n_tiles), tile = (int)(blockIdx.x % (unsigned)n_tiles);
  float* o = out + (int64_t)n * hw;
  double c0 = 1.0, c1 = 0.0;
  const bool fit = ref.steps != nullptr;
  if (fit) {
    const double* src = ref.steps + ((size_t)n * ref.n_steps + ref.step0) * 2;
    c0 = src[0];
    c1 = src[1];
  }
  float lo = __builtin_inff(), hi = -__builtin_inff();
#pragma unroll
  for (int k = 0; k < HRC_EPT; ++k) {
    const int e = tile * HRC_TILE + k * HRC_THREADS + t;
    if (e < hw) {
      float v = o[e];
      if (fit) {
        v = (float)(c0 * (double)v + c1);
        o[e] = v;
      }
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, d, 64));
    hi = fmaxf(hi, __shfl_xor(hi, d, 64));
  }
  if (lane == 0) {
    red[wave][0] = lo;
    red[wave][1] = hi;
  }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int w = 1; w < HRC_WAVES; ++w) {
      lo = fminf(lo, red[w][0]);
      hi = fmaxf(hi, red[w][1]);
    }
    part[(size_t)blockIdx.x * 2] = (double)lo;
    part[(size_t)blockIdx.x * 2 + 1] = (double)hi;
  }
}

// min and max are exact: any order gives the same result
__global__ void __launch_bounds__(MSDF_WAVE)
hrc_depth_minmax_k(const double* __restrict__ part, int n_tiles, double* __restrict__ mm) {
  const int n = (int)blockIdx.x, lane = lane_id();
  double lo = __builtin_inf(), hi = -__builtin_inf();
  for (int tile = lane; tile < n_tiles; tile += MSDF_WAVE) {
    lo = fmin(lo, part[((size_t)n * n_tiles + tile) * 2]);
    hi = fmax(hi, part[((size_t)n * n_tiles + tile) * 2 + 1]);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    lo = fmin(lo, __shfl_xor(lo, d, 64));
    hi = fmax(hi, __shfl_xor(hi, d, 64));
  }
  if (lane == 0) {
    mm[2 * n] = lo;
    mm[2 * n + 1] = hi;
  }
}

__global__ void __launch_bounds__(HRC_THREADS)
hrc_depth_normalize_k(float* __restrict__ out, int hw, int n_tiles, const double* __restrict__ mm) {
  const int n = (int)(blockIdx.x / (unsigned)n_tiles), tile = (int)(blockIdx.x % (unsigned)n_tiles);
  float* o = out + (int64_t)n * hw;
  const double lo = mm[2 * n], range = mm[2 * n + 1] - lo;
#pragma unroll
  for (int k = 0; k < HRC_EPT; ++k) {
    const int e = tile * HRC_TILE + k * HRC_THREADS + (int)threadIdx.x;
    if (e < hw) o[e] = (float)(((double)o[e] - lo) / range);
  }
}

// normals: out = R out where a centre fit was made, then (out + 1) / 2
__global__ void __launch_bounds__(HRC_THREADS)
hrc_normal_encode_k(double* __restrict__ out, int hw, int n_tiles, HrcStepRef ref) {
  const int n = (int)(blockIdx.x / (unsigned)n_tiles), tile = (int)(blockIdx.x % (unsigned)n_tiles);
  double* o = out + (int64_t)n * 3 * hw;
  const bool fit = ref.steps != nullptr;
  double c[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) c[k] = 0.0;
  if (fit) {
    const double* src = ref.steps + ((size_t)n * ref.n_steps + ref.step0) * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) c[k] = src[k];
  }
#pragma unroll
  for (int k = 0; k < HRC_EPT; ++k) {
    const int e = tile * HRC_TILE + k * HRC_THREADS + (int)threadIdx.x;
    if (e >= hw) continue;
    double v[3] = {o[e], o[e + hw], o[e + 2 * (int64_t)hw]};
    if (fit) {
      const double x = v[0], y = v[1], z = v[2];
#pragma unroll
      for (int a = 0; a < 3; ++a) v[a] = (c[3 * a] * x + c[3 * a + 1] * y) + c[3 * a + 2] * z;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) o[e + a * (int64_t)hw] = (v[a] + 1.0) / 2.0;
  }
}

// ---------------------------------------------------------------- host side

inline int64_t hrc_tiles(int64_t elements) { return blocks_for(elements, HRC_TILE); }

struct HrcSizes {
  int64_t N, R, C, P, S, O, H, W, ch;
  int64_t part_doubles, strip_elems;                    // workspace: partial sums (+ 2 N for min, max), row strips
};

bool hrc_sizes(int64_t n, int64_t rows, int64_t cols, int64_t patch, int64_t stride, int64_t channels, HrcSizes& z) {
  if (channels != 1 && channels != 3) return false;
  if (n < 1 || n > 65536 || rows < 1 || rows > 1024 || cols < 1 || cols > 1024) return false;
  if (patch > 16384 || stride < 1 || stride >= patch || patch - stride < 2) return false;
  z.N = n, z.R = rows, z.C = cols, z.P = patch, z.S = stride, z.O = patch - stride, z.ch = channels;
  z.H = patch + stride * (rows - 1);
  z.W = patch + stride * (cols - 1);
  if (3 * z.H * z.W >= MSDF_COUNT_MAX) return false;                    // H, W < 2^25, so the product is below 2^52
  if (3 * n * rows * cols * patch * patch >= (1ll << 40)) return false; // factors below 2^2 2^17 2^10 2^10 2^28
  // workgroups per launch: the largest are the apply launches of the two phases and the last kernels
  const int64_t row = n * rows * hrc_tiles(patch * patch), col = n * hrc_tiles(patch * z.W), end = n * hrc_tiles(z.H * z.W);
  if (row >= MSDF_COUNT_MAX || col >= MSDF_COUNT_MAX || end >= MSDF_COUNT_MAX) return false;
  const int64_t ns = channels == 1 ? 4 : 9;
  int64_t part = n * rows * hrc_tiles(z.O * patch) * ns;
  if (n * hrc_tiles(z.O * z.W) * ns > part) part = n * hrc_tiles(z.O * z.W) * ns;
  if (n * hrc_tiles(patch * patch) * ns > part) part = n * hrc_tiles(patch * patch) * ns;
  if (end * 2 > part) part = end * 2;
  z.part_doubles = part + 2 * n;
  z.strip_elems = n * (rows - 1) * channels * patch * z.W;
  return true;
}

template <int NCH>
int hrc_merge(const typename HrcCue<NCH>::T* patches, const typename HrcCue<NCH>::T* mid, const HrcSizes& z,
              int normalize, void* workspace, typename HrcCue<NCH>::T* out, double* steps, hipStream_t st) {
  typedef typename HrcCue<NCH>::T T;
  typedef HrcView<T> View;
  const int64_t N = z.N, R = z.R, C = z.C, P = z.P, S = z.S, O = z.O, H = z.H, W = z.W;
  const int n_steps = (int)(R * (C - 1) + (R - 1) + (mid ? 1 : 0));
  double* part = (double*)workspace;
  double* mm = part + (z.part_doubles - 2 * N);
  T* strips = (T*)(part + z.part_doubles);
  T* in = const_cast<T*>(patches);
  const double wstep = -1.0 / (double)(O - 1);
  const int64_t PP = P * P, strip = NCH * P * W;

  // rows: step c moves every (image, row) chain one patch to the right; strip 0 of an image is built in `out`
  for (int64_t c = 0; c < C; ++c) {
    const View qv = {in, nullptr, R * C * NCH * PP, C * NCH * PP, PP, 0, 0, 1, P, c * NCH * PP};
    const View mv = {strips, out, (R - 1) * strip, strip, P * W, NCH * H * W, H * W, 1, W, c * S};
    const int chains = (int)(N * R);
    const HrcGeom ga = {(int)R, (int)P, (int)P, 1, (int)hrc_tiles(PP)};
    if (c == 0) {
      hrc_apply_k<NCH><<<(unsigned)(chains * ga.n_tiles), HRC_THREADS, 0, st>>>(qv, mv, ga, 0, wstep,
                                                                                 HrcStepRef{nullptr, 0, 0, 0});
      continue;
    }
    const HrcGeom gr = {(int)R, (int)O, (int)P, 1, (int)hrc_tiles(O * P)};
    const HrcStepRef ref = {steps, n_steps, (int)(c - 1), (int)(C - 1)};
    hrc_reduce_k<NCH><<<(unsigned)(chains * gr.n_tiles), HRC_THREADS, 0, st>>>(qv, mv, gr, part);
    hrc_solve_k<NCH><<<(unsigned)chains, MSDF_WAVE, 0, st>>>(part, gr.n_tiles, (int)R, (double)(O * P), ref);
    hrc_apply_k<NCH><<<(unsigned)(chains * ga.n_tiles), HRC_THREADS, 0, st>>>(qv, mv, ga, (int)O, wstep, ref);
    if constexpr (NCH == 3) {
      if (c == 1) {                                      // the first S columns of every row's first patch
        View head = mv;
        head.off = 0;
        const HrcGeom gh = {(int)R, (int)S, (int)P, 1, (int)hrc_tiles(S * P)};
        hrc_renorm_k<<<(unsigned)(chains * gh.n_tiles), HRC_THREADS, 0, st>>>(head, gh);
      }
    }
  }
  // columns: strip r of the workspace into the mosaic in `out`
  for (int64_t r = 1; r < R; ++r) {
    View qv = {strips, nullptr, (R - 1) * strip, 0, P * W, 0, 0, W, 1, (r - 1) * strip};
    View mv = {out, nullptr, NCH * H * W, 0, H * W, 0, 0, W, 1, r * S * W};
    HrcGeom gr = {1, (int)O, (int)W, 0, (int)hrc_tiles(O * W)}, ga = {1, (int)P, (int)W, 0, (int)hrc_tiles(P * W)};
    HrcStepRef ref = {steps, n_steps, (int)(R * (C - 1) + r - 1), 0};
    hrc_reduce_k<NCH><<<(unsigned)(N * gr.n_tiles), HRC_THREADS, 0, st>>>(qv, mv, gr, part);
    hrc_solve_k<NCH><<<(unsigned)N, MSDF_WAVE, 0, st>>>(part, gr.n_tiles, 1, (double)(O * W), ref);
    hrc_apply_k<NCH><<<(unsigned)(N * ga.n_tiles), HRC_THREADS, 0, st>>>(qv, mv, ga, (int)O, wstep, ref);
    if constexpr (NCH == 3) {
      if (r == 1 && C == 1) {                            // no row step has met the first S rows of the first patch
        View head = mv;
        head.off = 0;
        const HrcGeom gh = {1, (int)S, (int)W, 0, (int)hrc_tiles(S * W)};
        hrc_renorm_k<<<(unsigned)(N * gh.n_tiles), HRC_THREADS, 0, st>>>(head, gh);
      }
    }
  }
  if constexpr (NCH == 3) {
    if (R == 1 && C == 1) {                              // no step at all: the one patch is divided on its own
      const View whole = {out, nullptr, NCH * H * W, 0, H * W, 0, 0, W, 1, 0};
      const HrcGeom gh = {1, (int)H, (int)W, 0, (int)hrc_tiles(H * W)};
      hrc_renorm_k<<<(unsigned)(N * gh.n_tiles), HRC_THREADS, 0, st>>>(whole, gh);
    }
  }
  // centre: the crop is p (A), mid is t (B)
  HrcStepRef fit = {nullptr, n_steps, n_steps - 1, 0};
  if (mid) {
    View pv = {out, nullptr, NCH * H * W, 0, H * W, 0, 0, W, 1, (H / 2 - P / 2) * W + (W / 2 - P / 2)};
    View tv = {const_cast<T*>(mid), nullptr, NCH * PP, 0, PP, 0, 0, P, 1, 0};
    HrcGeom gr = {1, (int)P, (int)P, 0, (int)hrc_tiles(PP)};
    fit.steps = steps;
    hrc_reduce_k<NCH><<<(unsigned)(N * gr.n_tiles), HRC_THREADS, 0, st>>>(pv, tv, gr, part);
    hrc_solve_k<NCH><<<(unsigned)N, MSDF_WAVE, 0, st>>>(part, gr.n_tiles, 1, (double)PP, fit);
  }
  const int hw = (int)(H * W), end_tiles = (int)hrc_tiles(H * W);
  if constexpr (NCH == 1) {
    if (mid || normalize)
      hrc_depth_affine_k<<<(unsigned)(N * end_tiles), HRC_THREADS, 0, st>>>(out, hw, end_tiles, fit, part);
    if (normalize) {
      hrc_depth_minmax_k<<<(unsigned)N, MSDF_WAVE, 0, st>>>(part, end_tiles, mm);
      hrc_depth_normalize_k<<<(unsigned)(N * end_tiles), HRC_THREADS, 0, st>>>(out, hw, end_tiles, mm);
    }
  } else {
    hrc_normal_encode_k<<<(unsigned)(N * end_tiles), HRC_THREADS, 0, st>>>(out, hw, end_tiles, fit);
  }
  return msdf_check_launch();
}

}  // namespace

extern "C" int64_t msdf_hrc_workspace_bytes(int64_t n, int64_t rows, int64_t cols, int64_t patch, int64_t stride,
                                            int64_t channels) {
  HrcSizes z;
  if (!hrc_sizes(n, rows, cols, patch, stride, channels, z)) return -1;
  return z.part_doubles * 8 + z.strip_elems * (channels == 1 ? 4 : 8) + 256;
}

extern "C" int msdf_hrc_merge_depth(const float* patches, const float* mid, int64_t n, int64_t rows, int64_t cols,
                                    int64_t patch, int64_t stride, int normalize, void* workspace, float* out,
                                    double* steps, void* stream) {
  HrcSizes z;
  if (!hrc_sizes(n, rows, cols, patch, stride, 1, z)) return MSDF_ERR_ARG;
  const int64_t n_steps = rows * (cols - 1) + (rows - 1) + (mid ? 1 : 0);
  if (!patches || !workspace || !out || (n_steps > 0 && !steps)) return MSDF_ERR_ARG;
  return hrc_merge<1>(patches, mid, z, normalize, workspace, out, steps, (hipStream_t)stream);
}

extern "C" int msdf_hrc_merge_normals(const double* patches, const double* mid, int64_t n, int64_t rows, int64_t cols,
                                      int64_t patch, int64_t stride, void* workspace, double* out, double* steps,
                                      void* stream) {
  HrcSizes z;
  if (!hrc_sizes(n, rows, cols, patch, stride, 3, z)) return MSDF_ERR_ARG;
  const int64_t n_steps = rows * (cols - 1) + (rows - 1) + (mid ? 1 : 0);
  if (!patches || !workspace || !out || (n_steps > 0 && !steps)) return MSDF_ERR_ARG;
  return hrc_merge<3>(patches, mid, z, 0, workspace, out, steps, (hipStream_t)stream);
}
