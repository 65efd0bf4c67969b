// The embedding-table gradient of the hash grid ("scatter"): its three forms -- one float atomic per corner
// (hg_scatter_*), binned with exact bin sizes (hb_*), binned with fixed regions (hb2_*: what the training step runs) --
// and the one host launcher that chooses between them, hg_table_gradient.  Included by hashgrid.hip alone, after the
// cell and level helpers the kernels use (HgCell, HgLevel, hg_locate, hg_corner_index, HgCorners): one translation unit,
// its -ffp-contract=off.  The three forms differ only in how a corner's value reaches the table: which value goes to
// which entry is hg_corner_value and hg_corner_index for all of them; the binned forms share the record (hb_write_record /
// hb_read_record), the block scan (hb_block_scan) and the flush of a summed slice (hb_flush_slice).
#pragma once

// ---------------------------------------------------------------------------
// grid backward and second backward (embedding): scatter into the 8 corners (float atomics, like the
// reference; one code path for both kernels, they differ in the per-corner coefficient only).
// Lane mapping: C consecutive lanes own the C channels of ONE (point, level), so a wave-instruction
// adds 64/C entries of C contiguous floats each -- half (C=2) as many distinct memory segments per
// instruction as one-point-per-lane, which is what the memory-side atomic units are paced by
// (MI355X_MICROARCH.md "Global float atomics", access-shape row).
// ---------------------------------------------------------------------------
// value added to corner k of (point b, level, channel ch): hg_corner_value<SECOND> (MODE 0: kernel_grid_backward,
// MODE 1: kernel_grid_second_backward_embedding), at entry hg_corner_index.
// levels [level_base, level_base + gridDim.y): straight to memory
template <int C, bool SECOND>
__global__ void __launch_bounds__(HG_THREADS)
hg_scatter_kernel(const float* __restrict__ grad, const float* __restrict__ inputs, const int* __restrict__ offsets,
                  const float* __restrict__ gg_inputs, float* __restrict__ grad_grid, const uint32_t B,
                  const uint32_t level_base, const float S, const uint32_t H) {
  const uint32_t t = blockIdx.x * HG_THREADS + threadIdx.x;
  const uint32_t b = t / C, ch = t % C;
  if (b >= B) return;
  const uint32_t level = level_base + blockIdx.y;
  const HgLevel lv = hg_level(offsets, level, S, H);
  const HgCell c = hg_locate(inputs, lv, b);
  if (c.oob) return;
  const float g = grad[((size_t)level * B + b) * C + ch];
  float* table = grad_grid + (size_t)(uint32_t)offsets[level] * C + ch;
  const HgCorners cn(c, SECOND ? gg_inputs + (size_t)b * 3 : nullptr);
  float val[8];
  uint32_t idx[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    val[k] = hg_corner_value<SECOND ? 1 : 0>(cn.weight(k), cn.coefficient(k), g, 0.f);
    idx[k] = hg_corner_index(lv, c, k);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) unsafeAtomicAdd(table + (size_t)idx[k] * C, val[k]);
}

// The coarsest levels (4,096 and 12,167 entries for the 16 -> 2048 pyramid) take every point of the batch, so
// hundreds of atomics land on each entry and serialise at the memory-side atomic units: alone, level 0 costs
// 5x and level 1 3x a fine level (scripts/diag_hash_levels.py).  Their whole table fits in LDS, so a workgroup
// accumulates its share of the points with LDS atomics and adds the non-zero entries to memory once.
#define HG_LDS_THREADS 1024
#define HG_LDS_WGS 128                     // workgroups per level
#define HG_LDS_MAX_BYTES (100 * 1024)

template <int C, bool SECOND>
__global__ void __launch_bounds__(HG_LDS_THREADS)
hg_scatter_lds_kernel(const float* __restrict__ grad, const float* __restrict__ inputs,
                      const int* __restrict__ offsets, const float* __restrict__ gg_inputs,
                      float* __restrict__ grad_grid, const uint32_t B, const float S, const uint32_t H,
                      const uint32_t lds_floats) {
  extern __shared__ float hg_tab[];
  const uint32_t level = blockIdx.y;
  const HgLevel lv = hg_level(offsets, level, S, H);
  const uint32_t n = lv.hsize * C;
  const bool in_lds = n <= lds_floats;       // host-side sizing is an estimate: fall back if the level is larger
  float* table = grad_grid + (size_t)(uint32_t)offsets[level] * C;
  // LDS atomics (~64 lanes per 32 cycles per CU, several same-address lanes per instruction on these levels) are
  // what bounds a workgroup, so the level is spread over many of them; each flushes only the entries its few
  // rays touched (the non-zero ones), which keeps the memory-side adds far below the direct count
  const uint32_t n_wg = gridDim.x;
  if (in_lds) {
    for (uint32_t i = threadIdx.x; i < n; i += HG_LDS_THREADS) hg_tab[i] = 0.f;
    __syncthreads();
  }
  const uint32_t per = (B + n_wg - 1) / n_wg;
  const uint32_t b_end = min(B, (blockIdx.x + 1) * per);
  for (uint32_t t = blockIdx.x * per * C + threadIdx.x; t < b_end * C; t += HG_LDS_THREADS) {
    const uint32_t b = t / C, ch = t % C;
    const HgCell c = hg_locate(inputs, lv, b);
    if (c.oob) continue;
    const float g = grad[((size_t)level * B + b) * C + ch];
    const HgCorners cn(c, SECOND ? gg_inputs + (size_t)b * 3 : nullptr);
    float val[8];
    uint32_t idx[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      val[k] = hg_corner_value<SECOND ? 1 : 0>(cn.weight(k), cn.coefficient(k), g, 0.f);
      idx[k] = hg_corner_index(lv, c, k);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (in_lds) atomicAdd(&hg_tab[idx[k] * C + ch], val[k]);
      else unsafeAtomicAdd(table + (size_t)idx[k] * C + ch, val[k]);
    }
  }
  if (in_lds) {
    __syncthreads();
    // every workgroup starts its flush at a different entry, so they do not walk the table in lockstep
    const uint32_t start = (uint32_t)(((uint64_t)blockIdx.x * n) / n_wg);
    for (uint32_t i = threadIdx.x; i < n; i += HG_LDS_THREADS) {
      uint32_t e = i + start;
      e = (e >= n) ? e - n : e;
      const float v = hg_tab[e];
      if (v != 0.f) unsafeAtomicAdd(table + e, v);
    }
  }
}

// number of leading levels whose dense table fits the LDS budget, from the kernels' own resolution formula
static uint32_t hg_small_levels(const uint32_t C, const uint32_t L, const float S, const uint32_t H, uint32_t* lds_bytes) {
  uint32_t n = 0, bytes = 0;
  for (uint32_t l = 0; l < L; ++l) {
    const double res = (double)hg_resolution(l, S, H).res;
    const double b = res * res * res * C * 4.0;
    if (b > (double)HG_LDS_MAX_BYTES) break;
    bytes = (uint32_t)b > bytes ? (uint32_t)b : bytes;
    ++n;
  }
  *lds_bytes = (bytes + 255u) & ~255u;
  return n;
}

template <int C, bool SECOND>
static int hg_launch_scatter(const float* grad, const float* inputs, const int* offsets, const float* gg_inputs,
                             float* grad_grid, const uint32_t B, const uint32_t L, const float S, const uint32_t H,
                             hipStream_t st) {
  uint32_t lds_bytes = 0;
  const uint32_t n_small = hg_small_levels(C, L, S, H, &lds_bytes);
  if (n_small > 0) {
    if (hipFuncSetAttribute((const void*)hg_scatter_lds_kernel<C, SECOND>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds_bytes) != hipSuccess)
      return MSDF_ERR_LAUNCH;
    hg_scatter_lds_kernel<C, SECOND><<<dim3(HG_LDS_WGS, n_small), HG_LDS_THREADS, lds_bytes, st>>>(
        grad, inputs, offsets, gg_inputs, grad_grid, B, S, H, lds_bytes / 4);
  }
  if (L > n_small) {
    const dim3 grid_c((B * C + HG_THREADS - 1) / HG_THREADS, L - n_small);   // one lane per (point, channel)
    hg_scatter_kernel<C, SECOND><<<grid_c, HG_THREADS, 0, st>>>(grad, inputs, offsets, gg_inputs, grad_grid, B, n_small,
                                                                S, H);
  }
  return MSDF_OK;
}

// ---------------------------------------------------------------------------
// Binned scatter: the same sums WITHOUT one memory-side atomic per corner.
//
// The direct kernels above issue B * L * 8 scattered float-atomic requests per call; the memory-side atomic units
// retire ~20 G requests/s whatever the schedule (MI355X_MICROARCH.md "Global float atomics": one 64-B request per
// distinct row), which is where they sit (0.59 ms for the 14 fine levels at B = 104,448).  Here every level's table
// is cut into slices of HB_SLICE_FLOATS floats (one LDS accumulator), and
//   hb_count_k       counts the corner contributions per (level, slice) bin      [LDS histogram per workgroup]
//   hb_scan_k        turns the counts into bin offsets and a list of work items  [one workgroup]
//   hb_place_k       writes each contribution as a record {entry in slice, C values} into its bin
//   hb_accumulate_k  one workgroup per bin (or per HB_CHUNK records of a crowded bin) sums its records into LDS
//                    with ds_add_f32 and adds the slice to the table once: plain read-modify-write when the
//                    bin has one workgroup, contiguous float atomics (the fast shape) when it has several.
// Coarse levels (hundreds of contributions per entry) and fine hashed levels (mostly unique entries) take the same
// path; the records are the only extra traffic (B * L * 8 * (4 + 4 C) bytes written once, read once).
// The sum order inside a bin follows the order in which workgroups reserved their runs: like the atomics it replaces
// it is not fixed from run to run (differences at fp32 rounding).
// ---------------------------------------------------------------------------
#ifndef HB_SLICE_FLOATS
#define HB_SLICE_FLOATS 8192
#endif
#define HB_CHUNK 8192
#define HB_THREADS 256
#define HB_PTS 4                      // points per thread in the count / place kernels (1,024 per workgroup)
#define HB_MAX_SLICES 1024            // per level, in the LDS histogram (2^19 entries x C = 8 -> 512)
#define HB_RANK_SHIFT 19              // first form: a corner between the place kernel's phases is (index | rank << 19)
#define HB_HDR_INTS 16
#define HB_REGION_RECORDS (8 * HB_PTS * HB_THREADS)   // corners of one place workgroup: the second form's fixed region

// A record is {entry in slice, C floats}: 1 + C dwords at position `pos` of a record array.
__host__ __device__ constexpr uint32_t hb_record_dwords(const uint32_t C) { return 1 + C; }
template <int C>
__device__ __forceinline__ void hb_write_record(uint32_t* __restrict__ rec, const size_t pos, const uint32_t entry,
                                                const float (&v)[C]) {
  uint32_t* r = rec + pos * hb_record_dwords(C);
  r[0] = entry;
#pragma unroll
  for (int ch = 0; ch < C; ++ch) r[1 + ch] = __float_as_uint(v[ch]);
}
template <int C>
__device__ __forceinline__ void hb_read_record(const uint32_t* __restrict__ rec, const size_t pos, uint32_t& entry,
                                               float (&v)[C]) {
  const uint32_t* r = rec + pos * hb_record_dwords(C);
  entry = r[0];
#pragma unroll
  for (int ch = 0; ch < C; ++ch) v[ch] = __uint_as_float(r[1 + ch]);
}

// Inclusive scan of a[0 .. N) in LDS, in place, by the N threads of a workgroup (t = its thread index; Hillis-Steele).
// A barrier stands between the caller's writes of a[] and the call; the result is visible to all threads on return.
template <int N>
__device__ __forceinline__ void hb_block_scan(int* a, const int t) {
  for (int d = 1; d < N; d <<= 1) {
    const int x = (t >= d) ? a[t - d] : 0;
    __syncthreads();
    a[t] += x;
    __syncthreads();
  }
}

struct HbLayout {                      // int32 offsets into the workspace
  int nb_max, work_max, slice_base, bin_count, bin_base, bin_cursor, work, hdr_ints;
  size_t rec_off_bytes, total_bytes;
};
static HbLayout hb_layout(const uint32_t B, const uint32_t C, const uint32_t L, const uint64_t n_entries) {
  HbLayout y;
  y.nb_max = (int)((n_entries * C + HB_SLICE_FLOATS - 1) / HB_SLICE_FLOATS + L);
  y.work_max = y.nb_max + (int)(((uint64_t)B * L * 8 + HB_CHUNK - 1) / HB_CHUNK);
  y.slice_base = HB_HDR_INTS;
  y.bin_count = y.slice_base + (int)L + 1;
  y.bin_base = y.bin_count + y.nb_max;
  y.bin_cursor = y.bin_base + y.nb_max + 1;
  y.work = (y.bin_cursor + y.nb_max + 3) & ~3;          // int4 descriptors, 16-byte aligned
  y.hdr_ints = y.work + 4 * y.work_max;
  y.rec_off_bytes = (((size_t)y.hdr_ints * 4) + 255) & ~(size_t)255;
  y.total_bytes = y.rec_off_bytes + (size_t)B * L * 8 * 4 * hb_record_dwords(C);
  return y;
}

__global__ void __launch_bounds__(HB_THREADS)
hb_setup_k(int* __restrict__ ws, const HbLayout y, const int* __restrict__ offsets, const uint32_t L, const uint32_t C) {
  for (int i = threadIdx.x; i < y.nb_max; i += HB_THREADS) ws[y.bin_count + i] = 0;
  if (threadIdx.x == 0) {
    const uint32_t epb = HB_SLICE_FLOATS / C;
    int base = 0;
    for (uint32_t l = 0; l < L; ++l) {
      ws[y.slice_base + l] = base;
      const uint32_t hsize = (uint32_t)(offsets[l + 1] - offsets[l]);
      base += (int)((hsize + epb - 1) / epb);
    }
    ws[y.slice_base + L] = base;
    ws[0] = base;                      // number of bins in use
  }
}

template <int C>
__global__ void __launch_bounds__(HB_THREADS)
hb_count_k(const float* __restrict__ inputs, const int* __restrict__ offsets, int* __restrict__ ws, const HbLayout y,
           const uint32_t B, const float S, const uint32_t H) {
  __shared__ int hist[HB_MAX_SLICES];
  const uint32_t level = blockIdx.y;
  const int sb = ws[y.slice_base + level];
  const int ns = ws[y.slice_base + level + 1] - sb;
  const bool local = ns <= HB_MAX_SLICES;
  if (local) {
    for (int i = threadIdx.x; i < ns; i += HB_THREADS) hist[i] = 0;
    __syncthreads();
  }
  constexpr uint32_t epb = HB_SLICE_FLOATS / C;
  const HgLevel lv = hg_level(offsets, level, S, H);
#pragma unroll
  for (int p = 0; p < HB_PTS; ++p) {
    const uint32_t b = (blockIdx.x * HB_PTS + p) * HB_THREADS + threadIdx.x;
    if (b >= B) continue;
    const HgCell c = hg_locate(inputs, lv, b);
    if (c.oob) continue;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint32_t idx = hg_corner_index(lv, c, k);
      const int s = (int)(idx / epb);
      if (local) atomicAdd(&hist[s], 1);
      else atomicAdd(&ws[y.bin_count + sb + s], 1);
    }
  }
  if (local) {
    __syncthreads();
    for (int i = threadIdx.x; i < ns; i += HB_THREADS) {
      const int n = hist[i];
      if (n) atomicAdd(&ws[y.bin_count + sb + i], n);
    }
  }
}

// exclusive scans over the bins: record offsets, and the list of work items for hb_accumulate_k -- one per
// HB_CHUNK records of a bin: {first record, end record, first float of the slice in the table, floats | shared flag}
__global__ void __launch_bounds__(1024)
hb_scan_k(int* __restrict__ ws, const HbLayout y, const int* __restrict__ offsets, const uint32_t L, const uint32_t C,
          const float S, const uint32_t H) {
  __shared__ int part[1024], partw[1024];
  const int nb = ws[0];
  const int t = threadIdx.x;
  const int per = (nb + 1023) / 1024;
  const int lo = min(nb, t * per), hi = min(nb, lo + per);
  int s = 0, w = 0;
  for (int i = lo; i < hi; ++i) {
    const int n = ws[y.bin_count + i];
    s += n;
    w += (n + HB_CHUNK - 1) / HB_CHUNK;
  }
  part[t] = s; partw[t] = w;
  __syncthreads();
  hb_block_scan<1024>(part, t);                   // the per-thread totals
  hb_block_scan<1024>(partw, t);
  int run = part[t] - s, runw = partw[t] - w;
  const uint32_t epb = HB_SLICE_FLOATS / C;
  int level = 0;
  for (int i = lo; i < hi; ++i) {
    const int n = ws[y.bin_count + i];
    ws[y.bin_base + i] = run;
    ws[y.bin_cursor + i] = run;
    while (level + 1 < (int)L && ws[y.slice_base + level + 1] <= i) ++level;
    const uint32_t e0 = (uint32_t)(i - ws[y.slice_base + level]) * epb;
    const uint32_t hsize = (uint32_t)(offsets[level + 1] - offsets[level]);
    const int nf = (int)(min(epb, hsize - e0) * C);
    const int chunks = (n + HB_CHUNK - 1) / HB_CHUNK;
    // hashed as the index function has it, by its 32-bit running stride (the flag only selects the LDS add of
    // hb_accumulate_k: no result depends on it)
    const bool hashed = !hg_level(offsets, (uint32_t)level, S, H).dense;
    for (int c = 0; c < chunks; ++c) {
      int* d = ws + y.work + 4 * (runw + c);
      d[0] = run + c * HB_CHUNK;
      d[1] = min(run + n, run + (c + 1) * HB_CHUNK);
      d[2] = (int)(((uint32_t)offsets[level] + e0) * C);   // < 2^31 floats: tables of up to 8 GB
      // bit 30: several workgroups share the slice; bit 29: hashed level (its records rarely repeat an entry)
      d[3] = nf | (chunks > 1 ? (int)0x40000000 : 0) | (hashed ? (int)0x20000000 : 0);
    }
    run += n;
    runw += chunks;
  }
  if (t == 1023) {
    ws[y.bin_base + nb] = part[1023];
    ws[1] = partw[1023];               // number of work items
  }
}

// MODE: which of its terms a record holds, hg_corner_value<MODE>.
// A workgroup takes 1,024 points of one level: phase 1 ranks every corner inside (workgroup, bin) with an LDS
// histogram, one returning global atomic per non-empty bin then reserves the workgroup's run in the bin, phase 2
// writes the records.  (index in level | rank << HB_RANK_SHIFT) is all that is kept per corner between the phases.
template <int C, int MODE>
__global__ void __launch_bounds__(HB_THREADS)
hb_place_k(const float* __restrict__ grad, const float* __restrict__ grad2, const float* __restrict__ inputs,
           const int* __restrict__ offsets, const float* __restrict__ gg_inputs, int* __restrict__ ws,
           const HbLayout y, const uint32_t B, const float S, const uint32_t H) {
  __shared__ int hist[HB_MAX_SLICES];
  const uint32_t level = blockIdx.y;
  const int sb = ws[y.slice_base + level];
  const int ns = ws[y.slice_base + level + 1] - sb;
  const HgLevel lv = hg_level(offsets, level, S, H);
  // packed (index | rank << 19) needs index < 2^19 and rank < 2^13 (HB_REGION_RECORDS = 8 * 1,024 per workgroup)
  const bool local = ns <= HB_MAX_SLICES && lv.hsize <= (1u << HB_RANK_SHIFT);
  if (local) {
    for (int i = threadIdx.x; i < ns; i += HB_THREADS) hist[i] = 0;
    __syncthreads();
  }
  constexpr uint32_t epb = HB_SLICE_FLOATS / C;
  uint32_t packed[HB_PTS][8];
#pragma unroll
  for (int p = 0; p < HB_PTS; ++p) {
    const uint32_t b = (blockIdx.x * HB_PTS + p) * HB_THREADS + threadIdx.x;
    if (b >= B) continue;
    const HgCell c = hg_locate(inputs, lv, b);
    if (c.oob) continue;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint32_t idx = hg_corner_index(lv, c, k);
      const int s = (int)(idx / epb);
      if (local) packed[p][k] = idx | ((uint32_t)atomicAdd(&hist[s], 1) << HB_RANK_SHIFT);
      else packed[p][k] = (uint32_t)atomicAdd(&ws[y.bin_cursor + sb + s], 1);     // absolute record position
    }
  }
  if (local) {
    __syncthreads();
    for (int i = threadIdx.x; i < ns; i += HB_THREADS) {
      const int n = hist[i];
      hist[i] = n ? atomicAdd(&ws[y.bin_cursor + sb + i], n) : 0;       // start of this workgroup's run
    }
    __syncthreads();
  }
  uint32_t* rec = (uint32_t*)((char*)ws + y.rec_off_bytes);
#pragma unroll
  for (int p = 0; p < HB_PTS; ++p) {
    const uint32_t b = (blockIdx.x * HB_PTS + p) * HB_THREADS + threadIdx.x;
    if (b >= B) continue;
    const HgCell c = hg_locate(inputs, lv, b);
    if (c.oob) continue;
    const HgCorners cn(c, MODE != 0 ? gg_inputs + (size_t)b * 3 : nullptr);
    float g1[C], g2[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      g1[ch] = grad[((size_t)level * B + b) * C + ch];
      g2[ch] = (MODE == 2) ? grad2[((size_t)level * B + b) * C + ch] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float wk = cn.weight(k), qk = cn.coefficient(k);
      uint32_t idx, pos;
      if (local) {
        idx = packed[p][k] & ((1u << HB_RANK_SHIFT) - 1);
        pos = (uint32_t)hist[idx / epb] + (packed[p][k] >> HB_RANK_SHIFT);
      } else {
        idx = hg_corner_index(lv, c, k);
        pos = packed[p][k];
      }
      float v[C];
#pragma unroll
      for (int ch = 0; ch < C; ++ch) v[ch] = hg_corner_value<MODE>(wk, qk, g1[ch], g2[ch]);
      hb_write_record<C>(rec, pos, idx % epb, v);
    }
  }
}

// acc += v in LDS as a compare-and-swap loop (for addresses that rarely collide)
__device__ __forceinline__ void lds_add_cas(float* p, const float v) {
  uint32_t* u = (uint32_t*)p;
  uint32_t old = *u;
  while (true) {
    // the sum goes through an opaque instruction: left visible, the compiler recognises the loop as an atomic float
    // add and turns it back into ds_add_f32
    float sum;
    asm volatile("v_add_f32 %0, %1, %2" : "=v"(sum) : "v"(__uint_as_float(old)), "v"(v));
    const uint32_t got = atomicCAS(u, old, __float_as_uint(sum));
    if (got == old) break;
    old = got;
  }
}

// The tail of both accumulate kernels: the slice summed in LDS goes to its `ne` entries of the table.  acc(i, ch) reads
// channel ch of entry i from the accumulator (the two forms lay it out differently).
template <int C, typename Acc>
__device__ __forceinline__ void hb_flush_slice(float* __restrict__ table, const uint32_t ne, const bool shared_slice,
                                               const bool overwrite, const Acc acc) {
  const uint32_t tid = threadIdx.x;
  if (shared_slice) {
    for (uint32_t i = tid; i < ne * C; i += HB_THREADS) {
      const float v = acc(i / C, i % C);
      if (v != 0.f) unsafeAtomicAdd(table + i, v);  // neighbouring lanes, neighbouring floats: the fast atomic shape
    }
    return;
  }
  // this workgroup owns the slice: plain read-modify-write, one entry (C floats) per lane and step.  Level offsets
  // are arbitrary entry counts (12,167 ...), so a table row is aligned to one entry, not to 16 bytes.
  typedef float vcf __attribute__((ext_vector_type(C)));
  vcf* tc = (vcf*)table;
  const auto entry = [&](const uint32_t i) {
    vcf a;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) a[ch] = acc(i, ch);
    return a;
  };
  if (overwrite) {                         // the table gradient is an output, not an accumulator: nothing to read
    for (uint32_t i = tid; i < ne; i += HB_THREADS) tc[i] = entry(i);
    return;
  }
  constexpr int UF = 8;
  for (uint32_t i0 = tid; i0 < ne; i0 += UF * HB_THREADS) {
    vcf t[UF];
    // all loads issued (index clamped to the last entry): a branch around a load makes the compiler wait for each one
    // in turn (cdna_hip_programming.md, "Projection GEMM" item 4c)
#pragma unroll
    for (int u = 0; u < UF; ++u) t[u] = tc[min(i0 + u * HB_THREADS, ne - 1)];
#pragma unroll
    for (int u = 0; u < UF; ++u) {
      const uint32_t i = i0 + u * HB_THREADS;
      if (i < ne) tc[i] = t[u] + entry(i);
    }
  }
}

template <int C>
__global__ void __launch_bounds__(HB_THREADS)
hb_accumulate_k(const int* __restrict__ ws, const HbLayout y, float* __restrict__ grad_grid) {
  __shared__ float acc[HB_SLICE_FLOATS];
  const int w = blockIdx.x;
  if (w >= ws[1]) return;
  const int4 d = *(const int4*)(ws + y.work + 4 * w);
  const int r0 = d.x, r1 = d.y;
  const uint32_t nf = (uint32_t)(d.w & 0x1fffffff);
  const bool shared_slice = (d.w & 0x40000000) != 0;
  const bool hashed = (d.w & 0x20000000) != 0;
  constexpr uint32_t epb = HB_SLICE_FLOATS / C;
  for (uint32_t i = threadIdx.x; i < HB_SLICE_FLOATS; i += HB_THREADS) acc[i] = 0.f;
  __syncthreads();
  const uint32_t* rec = (const uint32_t*)((const char*)ws + y.rec_off_bytes);
  // eight records per lane in flight: the loop is a chain of (HBM load -> LDS add) otherwise
  constexpr int U = 8;
  for (int i0 = r0 + (int)threadIdx.x; i0 < r1; i0 += U * HB_THREADS) {
    uint32_t e[U];
    float v[U][C];
    // every load is issued (index clamped to the last record): a branch around a load makes the compiler wait for
    // each one in turn (cdna_hip_programming.md, "Projection GEMM" item 4c)
#pragma unroll
    for (int u = 0; u < U; ++u) hb_read_record<C>(rec, (size_t)min(i0 + u * HB_THREADS, r1 - 1), e[u], v[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (i0 + u * HB_THREADS < r1) {
        // channel planes: the 64 lanes of one ds_add_f32 spread over all 32 banks.  These LDS float atomics are what
        // bounds the kernel (0.133 of its 0.155 ms at B = 104,448; loads 0.02, flush 0.005).  ds_add_f32 costs ~170
        // cycles per wave-instruction on gfx950 against 8 for ds_add_u32 (scripts/dbg/lds_atomics.hip); a
        // compare-and-swap loop is 7x faster in that microbenchmark but slower here when used for every level (0.30 ->
        // 0.38 ms per step: the ray samples' coarse-level records repeat entries, every repeat is a retry), so only
        // the hashed levels take it -- profiles/r02_hash_scatter.md
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
          if (hashed) lds_add_cas(&acc[ch * epb + e[u]], v[u][ch]);
          else atomicAdd(&acc[ch * epb + e[u]], v[u][ch]);
        }
      }
    }
  }
  __syncthreads();
  hb_flush_slice<C>(grad_grid + (size_t)(uint32_t)d.z, nf / C, shared_slice, false,
                    [&](const uint32_t i, const uint32_t ch) { return acc[ch * epb + i]; });
}

// ---------------------------------------------------------------------------
// Binned scatter, second form ("hb2", round 3): no counting pass, no scan kernel, no global cursors.
//
//   hb2_place_k       a workgroup takes 1,024 consecutive points of one level and owns a FIXED region of 8,192
//                     records: it counting-sorts its own corner contributions by table slice in LDS, writes them to
//                     its region in slice order and writes the (slices + 1) run offsets of the region to a run table
//                     [level][workgroup][slice].  Consecutive points that sit in the same cell (consecutive samples of
//                     a ray at the coarse levels) are summed on the way -- a segmented reduction over 16-lane rows with
//                     DPP -- so that one record leaves per run, not per point: fewer records, and the LDS adds of the
//                     second kernel rarely meet.
//   hb2_accumulate_k  one workgroup per (level, slice, group of place workgroups): reads the group's runs for its
//                     slice through the run table, adds them into an LDS accumulator with compare-and-swap float
//                     adds (both channels of an entry in one 64-bit swap; ds_add_f32 costs ~170 cycles per
//                     wave-instruction on gfx950, the swap loop ~25) and adds the slice to the table once.
// What the first form paid for exact bin sizes (hb_setup_k + hb_count_k + hb_scan_k, ~45 us of 255 at B = 104,448)
// is gone: the work list is a function of the level sizes alone.  Levels with few slices are cut by place workgroups
// instead (a coarse level of one slice becomes n_wg work items of one run each).
// ---------------------------------------------------------------------------
#define HB2_NS_MAX 8192               // slices per level the place kernel's LDS histogram is sized for
#define HB2_TILE 256                  // runs per pass of the accumulate kernel

struct Hb2Layout {
  int n_wg, ns_bound, rt_stride, work_max;
  size_t rec_off_bytes, total_bytes;
};
static Hb2Layout hb2_layout(const uint32_t B, const uint32_t C, const uint32_t L, const uint64_t n_entries) {
  Hb2Layout y;
  y.n_wg = (int)((B + HB_PTS * HB_THREADS - 1) / (HB_PTS * HB_THREADS));
  const uint64_t ns = (n_entries * C + HB_SLICE_FLOATS - 1) / HB_SLICE_FLOATS + 1;   // >= slices of any one level
  y.ns_bound = (int)(ns < (uint64_t)(1 << 30) ? ns : (uint64_t)(1 << 30));
  y.rt_stride = y.ns_bound + 1;
  // items of a level: slices x ceil(n_wg / min(slices, n_wg)) <= slices + n_wg
  y.work_max = (int)((n_entries * C + HB_SLICE_FLOATS - 1) / HB_SLICE_FLOATS + L) + (int)L * y.n_wg;
  y.rec_off_bytes = (((size_t)L * y.n_wg * y.rt_stride * 4) + 255) & ~(size_t)255;
  y.total_bytes = y.rec_off_bytes + (size_t)L * y.n_wg * HB_REGION_RECORDS * 4 * hb_record_dwords(C);
  return y;
}

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(const uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
#define DPP_ROW_SHL(n) (0x100 + (n))       // lane i reads lane i + n of its 16-lane row (0 past the row's end)
#define DPP_ROW_SHR(n) (0x110 + (n))       // lane i reads lane i - n

// v_i += v_{i+d} where lane i + d continues lane i's run (m = 1.0f) -- four steps sum a run into its first lane
template <int CN>
__device__ __forceinline__ void run_sum(float (&v)[CN], const float m1, const float m2, const float m4, const float m8) {
#pragma unroll
  for (int ch = 0; ch < CN; ++ch) {
    v[ch] = __builtin_fmaf(m1, __uint_as_float(dpp_u32<DPP_ROW_SHL(1)>(__float_as_uint(v[ch]))), v[ch]);
    v[ch] = __builtin_fmaf(m2, __uint_as_float(dpp_u32<DPP_ROW_SHL(2)>(__float_as_uint(v[ch]))), v[ch]);
    v[ch] = __builtin_fmaf(m4, __uint_as_float(dpp_u32<DPP_ROW_SHL(4)>(__float_as_uint(v[ch]))), v[ch]);
    v[ch] = __builtin_fmaf(m8, __uint_as_float(dpp_u32<DPP_ROW_SHL(8)>(__float_as_uint(v[ch]))), v[ch]);
  }
}

template <int C, int MODE>
__global__ void __launch_bounds__(HB_THREADS)
hb2_place_k(const float* __restrict__ grad, const float* __restrict__ grad2, const float* __restrict__ inputs,
            const int* __restrict__ offsets, const float* __restrict__ gg_inputs, int* __restrict__ ws,
            const Hb2Layout y, const uint32_t B, const float S, const uint32_t H, float* __restrict__ zero_grid,
            const uint32_t pitch) {       // pitch > 0: grad / grad2 are point-major [B, pitch] (level l, channel c at l C + c)
  extern __shared__ int hb2_lds[];
  int* hist = hb2_lds;                       // [ns]: counts, then run starts
  int* part = hb2_lds + y.ns_bound + 1;      // [HB_THREADS] scan scratch
  const uint32_t level = blockIdx.y;
  const HgLevel lv = hg_level(offsets, level, S, H);
  constexpr uint32_t epb = HB_SLICE_FLOATS / C;
  const int ns = (int)((lv.hsize + epb - 1) / epb);
  const int tid = threadIdx.x;
  const uint32_t lane = tid & 63;
  for (int i = tid; i < ns; i += HB_THREADS) hist[i] = 0;
  if (zero_grid != nullptr && ns < y.n_wg) {
    // "=" instead of "+=" (msdf_hash_encode_backward_fused_out): the slices of this level are shared by several
    // accumulate workgroups, which add with atomics -- the level is zeroed here, one share per place workgroup
    // (this kernel has finished before the accumulate kernel starts)
    const uint32_t nfl = lv.hsize * C, share = (nfl + y.n_wg - 1) / y.n_wg;
    float* t = zero_grid + (size_t)(uint32_t)offsets[level] * C;
    const uint32_t lo = blockIdx.x * share, hi = min(nfl, lo + share);
    for (uint32_t i = lo + tid; i < hi; i += HB_THREADS) t[i] = 0.f;
  }
  __syncthreads();

  // the gradient values of this thread's points are needed in phase 3 only, but they come from tensors the SDF kernels
  // wrote long before (cold: HBM latency): issued here, they arrive under phases 1 and 2
  float g1v[HB_PTS][C], g2v[HB_PTS][C], ggv[HB_PTS][3];
#pragma unroll
  for (int p = 0; p < HB_PTS; ++p) {
    const uint32_t b = (blockIdx.x * HB_PTS + p) * HB_THREADS + tid;
    const uint32_t bc = b < B ? b : B - 1;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      const size_t gi = pitch ? (size_t)bc * pitch + level * C + ch : ((size_t)level * B + bc) * C + ch;
      g1v[p][ch] = grad[gi];
      g2v[p][ch] = (MODE == 2) ? grad2[gi] : 0.f;
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) ggv[p][d] = (MODE != 0) ? gg_inputs[(size_t)bc * 3 + d] : 0.f;
  }

  // ---- phase 1: runs of equal cells, rank of every run head's corners inside (workgroup, slice) ----
  uint32_t rank2[HB_PTS][4];                 // two 13-bit ranks per word
  uint32_t rid[HB_PTS];                      // run id inside the 16-lane row (>= 1), 255 = no contribution
  uint32_t heads = 0;
#pragma unroll
  for (int p = 0; p < HB_PTS; ++p) {
    const uint32_t b = (blockIdx.x * HB_PTS + p) * HB_THREADS + tid;
    const HgCell c = hg_locate(inputs, lv, b < B ? b : B - 1);
    const bool live = b < B && !c.oob;
    const uint32_t k1 = live ? (c.gx | (c.gy << 16)) : 0xffffffffu, k2 = live ? c.gz : 0xffffffffu;
    const uint32_t p1 = dpp_u32<DPP_ROW_SHR(1)>(k1), p2 = dpp_u32<DPP_ROW_SHR(1)>(k2);
    const bool head = live && ((lane & 15) == 0 || p1 != k1 || p2 != k2);
    const uint64_t hb = __ballot(head);
    const uint32_t row = (uint32_t)(hb >> (lane & 48)) & 0xffffu;
    rid[p] = live ? (uint32_t)__popc(row & ((2u << (lane & 15)) - 1u)) : 255u;
    if (head) heads |= 1u << p;
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
      uint32_t r0 = 0, r1 = 0;
      if (head) {
        r0 = (uint32_t)atomicAdd(&hist[hg_corner_index(lv, c, k) / epb], 1);
        r1 = (uint32_t)atomicAdd(&hist[hg_corner_index(lv, c, k + 1) / epb], 1);
      }
      rank2[p][k >> 1] = r0 | (r1 << 16);
    }
  }
  __syncthreads();

  // ---- phase 2: exclusive scan of the slice counts -> run starts; the run table row of this workgroup ----
  {
    const int per = (ns + HB_THREADS - 1) / HB_THREADS;
    const int lo = min(ns, tid * per), hi = min(ns, lo + per);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += hist[i];
    part[tid] = sum;
    __syncthreads();
    hb_block_scan<HB_THREADS>(part, tid);
    int run = part[tid] - sum;
    int* rt = ws + ((size_t)level * y.n_wg + blockIdx.x) * y.rt_stride;
    for (int i = lo; i < hi; ++i) {
      const int n = hist[i];
      hist[i] = run;
      rt[i] = run;
      run += n;
    }
    if (tid == HB_THREADS - 1) rt[ns] = part[HB_THREADS - 1];
    __syncthreads();
  }

  // ---- phase 3: the records ----
  uint32_t* rec = (uint32_t*)((char*)ws + y.rec_off_bytes) +
                  ((size_t)level * y.n_wg + blockIdx.x) * HB_REGION_RECORDS * hb_record_dwords(C);   // this workgroup's region
#pragma unroll
  for (int p = 0; p < HB_PTS; ++p) {
    const uint32_t b = (blockIdx.x * HB_PTS + p) * HB_THREADS + tid;
    const uint32_t bc = b < B ? b : B - 1;
    const HgCell c = hg_locate(inputs, lv, bc);
    const bool live = rid[p] != 255u;
    // lane i + d continues lane i's run?  (run ids of live lanes are >= 1, a read past the row's end gives 0)
    const float m1 = (live && dpp_u32<DPP_ROW_SHL(1)>(rid[p]) == rid[p]) ? 1.f : 0.f;
    const float m2 = (live && dpp_u32<DPP_ROW_SHL(2)>(rid[p]) == rid[p]) ? 1.f : 0.f;
    const float m4 = (live && dpp_u32<DPP_ROW_SHL(4)>(rid[p]) == rid[p]) ? 1.f : 0.f;
    const float m8 = (live && dpp_u32<DPP_ROW_SHL(8)>(rid[p]) == rid[p]) ? 1.f : 0.f;
    // the operands of HgCorners as plain locals: through the struct the compiler packs the products of phase 3
    // differently and this kernel takes 93 instead of 86 VGPRs at C = 2, MODE 2 (84 instead of 76 at MODE 1, a wave less)
    const float wx[2] = {1.f - c.sx, c.sx}, wy[2] = {1.f - c.sy, c.sy}, wz[2] = {1.f - c.sz, c.sz};
    float q0 = 0.f, q1 = 0.f, q2 = 0.f;
    if (MODE != 0) {
      q0 = ggv[p][0] * c.dx * c.scale;
      q1 = ggv[p][1] * c.dy * c.scale;
      q2 = ggv[p][2] * c.dz * c.scale;
    }
    float g1[C], g2[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      g1[ch] = live ? g1v[p][ch] : 0.f;
      g2[ch] = (MODE == 2 && live) ? g2v[p][ch] : 0.f;
    }
    const bool head = (heads >> p) & 1u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float wk = hg_corner_weight(wx, wy, wz, k), qk = hg_corner_coefficient(wx, wy, wz, q0, q1, q2, k);
      float v[C];
#pragma unroll
      for (int ch = 0; ch < C; ++ch) v[ch] = hg_corner_value<MODE>(wk, qk, g1[ch], g2[ch]);
      run_sum<C>(v, m1, m2, m4, m8);
      if (head) {
        const uint32_t idx = hg_corner_index(lv, c, k);
        const uint32_t pos = (uint32_t)hist[idx / epb] + ((rank2[p][k >> 1] >> ((k & 1) * 16)) & 0xffffu);
        hb_write_record<C>(rec, pos, idx % epb, v);
      }
    }
  }
}

// entry e of the LDS accumulator += v[0..C): float adds as compare-and-swap loops, two channels per 64-bit swap
template <int C>
__device__ __forceinline__ void lds_add_entry(float* acc, const uint32_t e, const float (&v)[C]) {
  if (C == 1) {
    lds_add_cas(acc + e, v[0]);
  } else {
#pragma unroll
    for (int h = 0; h < C / 2; ++h) {
      unsigned long long* u = (unsigned long long*)(acc + (size_t)e * C + 2 * h);
      unsigned long long old = *u;
      while (true) {
        const float a = __uint_as_float((uint32_t)old) + v[2 * h];
        const float b = __uint_as_float((uint32_t)(old >> 32)) + v[2 * h + 1];
        const unsigned long long want = (unsigned long long)__float_as_uint(a) | ((unsigned long long)__float_as_uint(b) << 32);
        const unsigned long long got = atomicCAS(u, old, want);
        if (got == old) break;
        old = got;
      }
    }
  }
}

template <int C>
__global__ void __launch_bounds__(HB_THREADS)
hb2_accumulate_k(const int* __restrict__ ws, const Hb2Layout y, const int* __restrict__ offsets, const uint32_t L,
                 float* __restrict__ grad_grid, const int overwrite) {
  __shared__ __attribute__((aligned(16))) float acc[HB_SLICE_FLOATS];      // [entry][C]
  __shared__ int pre[HB2_TILE + 1], st[HB2_TILE];
  constexpr uint32_t epb = HB_SLICE_FLOATS / C;
  // work item -> (level, slice, group of place workgroups): a function of the level sizes alone
  int w = blockIdx.x;
  uint32_t level = 0, hsize = 0;
  int ns = 0, G = 0;
  for (; level < L; ++level) {
    hsize = (uint32_t)(offsets[level + 1] - offsets[level]);
    ns = (int)((hsize + epb - 1) / epb);
    G = min(ns, y.n_wg);
    const int items = (G > 0) ? ns * ((y.n_wg + G - 1) / G) : 0;
    if (w < items) break;
    w -= items;
  }
  if (level >= L) return;
  const int slice = w % ns, wg0 = (w / ns) * G, wg1 = min(y.n_wg, wg0 + G);
  const bool shared_slice = G < y.n_wg;
  const int tid = threadIdx.x;
  for (uint32_t i = tid; i < HB_SLICE_FLOATS / 4; i += HB_THREADS) ((v4f*)acc)[i] = (v4f){0.f, 0.f, 0.f, 0.f};
  const uint32_t* rec_all = (const uint32_t*)((const char*)ws + y.rec_off_bytes);
  for (int t0 = wg0; t0 < wg1; t0 += HB2_TILE) {
    // this pass's runs: start and length per place workgroup, inclusive scan of the lengths
    const int wg = t0 + tid;
    int s0 = 0, n = 0;
    if (tid < HB2_TILE && wg < wg1) {
      const int* r = ws + ((size_t)level * y.n_wg + wg) * y.rt_stride + slice;
      s0 = r[0];
      n = r[1] - s0;
    }
    __syncthreads();                       // previous pass done with pre / st (and the zero fill, first pass)
    st[tid] = s0;
    pre[tid + 1] = n;
    if (tid == 0) pre[0] = 0;
    __syncthreads();
    hb_block_scan<HB2_TILE>(pre + 1, tid);
    const int total = pre[HB2_TILE];
    constexpr int U = 4;
    for (int i0 = tid; i0 < total; i0 += U * HB_THREADS) {
      uint32_t e[U];
      float v[U][C];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = min(i0 + u * HB_THREADS, total - 1);       // every load issued (index clamped), adds guarded below
        int j = 0;                                                // largest j with pre[j] <= i
#pragma unroll
        for (int step = HB2_TILE / 2; step > 0; step >>= 1)
          if (pre[j + step] <= i) j += step;
        hb_read_record<C>(rec_all, ((size_t)level * y.n_wg + t0 + j) * HB_REGION_RECORDS + (size_t)(st[j] + i - pre[j]),
                          e[u], v[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (i0 + u * HB_THREADS < total) lds_add_entry<C>(acc, e[u], v[u]);
    }
  }
  __syncthreads();
  const uint32_t e0 = (uint32_t)slice * epb;
  hb_flush_slice<C>(grad_grid + ((size_t)(uint32_t)offsets[level] + e0) * C, min(epb, hsize - e0), shared_slice,
                    overwrite != 0, [&](const uint32_t i, const uint32_t ch) { return acc[i * C + ch]; });
}

// MSDF_HASH_BINNED_FORM=1 (read once per process) makes every binned call take the first form (count / scan / place /
// accumulate) for comparison runs; otherwise it is the path for tables of more than HB2_NS_MAX slices per level only.
// (Binned or atomic is the caller's choice of entry point: the Python layer's MSDF_HASH_SCATTER is not read here.)
static bool hb_force_first_form() {
  static const int v = [] { const char* e = getenv("MSDF_HASH_BINNED_FORM"); return (e && e[0] == '1') ? 1 : 0; }();
  return v != 0;
}

// ---- the one host launcher behind the seven table-gradient entry points of hashgrid.hip ----
struct HgTableGrad {                   // what to add into (or write to) the table gradient
  const float *grad_first, *grad_second, *gg_inputs;   // NULL = that term is absent (gg_inputs goes with grad_second)
  uint32_t pitch;                      // 0: level-major operands [L, B, C]; > 0: point-major rows of `pitch` floats
  bool overwrite;                      // "=" instead of "+="
  bool binned;                         // false: one float atomic per corner ("+=", level-major, one term per call)
  uint64_t n_entries;                  // binned: rows of the table, and the caller-owned workspace
  void* workspace;
  size_t workspace_bytes;
};

// the binned forms.  MODE of the place kernels: 0 first term only, 1 second only (its operand in the `grad` slot), 2 both
template <int C, int MODE>
static int hb_run(const HgTableGrad& t, const float* inputs, const int* offsets, float* grad_grid, const uint32_t B,
                  const uint32_t L, const float S, const uint32_t H, hipStream_t st) {
  if (t.n_entries * C >= (1ull << 31) || (uint64_t)B * L * 8 >= (1ull << 31)) return MSDF_ERR_UNSUPPORTED;
  const float* grad = (MODE == 1) ? t.grad_second : t.grad_first;
  const float* grad2 = (MODE == 2) ? t.grad_second : nullptr;
  int* ws = (int*)t.workspace;
  const auto workspace_holds = [&](const size_t bytes) {
    return t.workspace != nullptr && t.workspace_bytes >= bytes && !((uintptr_t)t.workspace & 15);
  };
  const Hb2Layout y2 = hb2_layout(B, C, L, t.n_entries);
  if (y2.ns_bound <= HB2_NS_MAX && !hb_force_first_form()) {
    if (!workspace_holds(y2.total_bytes)) return MSDF_ERR_ARG;
    const size_t lds = (size_t)(y2.ns_bound + 1 + HB_THREADS) * sizeof(int);
    hb2_place_k<C, MODE><<<dim3((unsigned)y2.n_wg, L), HB_THREADS, lds, st>>>(
        grad, grad2, inputs, offsets, t.gg_inputs, ws, y2, B, S, H, t.overwrite ? grad_grid : nullptr, t.pitch);
    hb2_accumulate_k<C><<<(unsigned)y2.work_max, HB_THREADS, 0, st>>>(ws, y2, offsets, L, grad_grid, t.overwrite ? 1 : 0);
    return MSDF_OK;
  }
  if (t.pitch != 0) return MSDF_ERR_UNSUPPORTED;      // the first form reads level-major gradients only
  if (t.overwrite && hipMemsetAsync(grad_grid, 0, (size_t)t.n_entries * C * sizeof(float), st) != hipSuccess) return MSDF_ERR_LAUNCH;
  const HbLayout y = hb_layout(B, C, L, t.n_entries);
  if (!workspace_holds(y.total_bytes)) return MSDF_ERR_ARG;
  const dim3 grid_pl((B + HB_PTS * HB_THREADS - 1) / (HB_PTS * HB_THREADS), L);
  hb_setup_k<<<1, HB_THREADS, 0, st>>>(ws, y, offsets, L, C);
  hb_count_k<C><<<grid_pl, HB_THREADS, 0, st>>>(inputs, offsets, ws, y, B, S, H);
  hb_scan_k<<<1, 1024, 0, st>>>(ws, y, offsets, L, C, S, H);
  hb_place_k<C, MODE><<<grid_pl, HB_THREADS, 0, st>>>(grad, grad2, inputs, offsets, t.gg_inputs, ws, y, B, S, H);
  hb_accumulate_k<C><<<(unsigned)y.work_max, HB_THREADS, 0, st>>>(ws, y, grad_grid);
  return MSDF_OK;
}

// Refusals, in this order, all before anything is launched (the table gradient is untouched by a refused call):
// grad_grid == NULL -> ARG;  B == 0 -> OK ("=": the table is zeroed);  no term, a NULL operand or pitch < L C -> ARG;
// a form that cannot do what is asked, a table or record count >= 2^31 -> UNSUPPORTED;  workspace -> ARG (hb_run).
template <int C>
static int hg_table_gradient(const HgTableGrad& t, const float* inputs, const int* offsets, float* grad_grid,
                             const uint32_t B, const uint32_t L, const float S, const uint32_t H, hipStream_t st) {
  if (grad_grid == nullptr) return MSDF_ERR_ARG;
  if (B == 0) {                        // no points: nothing to add; the "=" forms give an all-zero table
    if (!t.overwrite) return MSDF_OK;
    return hipMemsetAsync(grad_grid, 0, (size_t)t.n_entries * C * sizeof(float), st) == hipSuccess ? MSDF_OK : MSDF_ERR_LAUNCH;
  }
  const bool first = t.grad_first != nullptr, second = t.grad_second != nullptr;
  if ((!first && !second) || (second && t.gg_inputs == nullptr) || inputs == nullptr || offsets == nullptr ||
      (t.pitch != 0 && t.pitch < L * C))
    return MSDF_ERR_ARG;
  if (!t.binned) {
    if ((first && second) || t.overwrite || t.pitch != 0) return MSDF_ERR_UNSUPPORTED;
    return second ? hg_launch_scatter<C, true>(t.grad_second, inputs, offsets, t.gg_inputs, grad_grid, B, L, S, H, st)
                  : hg_launch_scatter<C, false>(t.grad_first, inputs, offsets, nullptr, grad_grid, B, L, S, H, st);
  }
  const auto run = (first && second) ? hb_run<C, 2> : second ? hb_run<C, 1> : hb_run<C, 0>;
  return run(t, inputs, offsets, grad_grid, B, L, S, H, st);
}
