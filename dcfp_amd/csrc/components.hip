// components.hip — 8-connected components of a class mask at the scaled, padded label size, and the k-th pixel of a
// component: the device half of the `resample` sampler's crop location (Base.py:203-222).
//
// Contract (bit for bit).  The grid of a sample is Hp x Wp; pixel (y, x) is foreground iff y < dst_h, x < dst_w and
// id_table[raw[row_map[y], col_map[x]]] == cls (the nearest-neighbour maps of the augmentation; padding is background).
// The label of a component is the smallest linear index y*Wp + x among its pixels (background: -1); components are
// numbered 1..C in ascending order of that label; the pixels of a component are ordered by linear index.
//
// Five launches on the caller's stream, none of which waits on another block (no grid barrier, no flags):
//   1 tile      64x64 tile per block: mask -> LDS, union-find by minimum in LDS, flatten; writes parent[p] (the tile's
//               min-index root of p, as a global linear index) and aux[p] (pixels of the tile-local component at its
//               root, 0 elsewhere)
//   2 merge     one lane per pixel on the first row / first column of a tile: union with its foreground neighbours
//               across the tile line (atomicMin on parent, agent-scope atomic loads while other blocks update it)
//   3 flatten   parent[p] <- root(p); sizes of tile-local components are added to their global root (integer
//               atomics); per 2048-pixel block, the number of roots
//   4 scan      one block per sample: exclusive scan of the per-block root counts, the component count
//   5 compact   roots in linear order and their pixel counts
// The root of a set is always its minimum index (a union links the larger root under the smaller), so the result does
// not depend on the order in which blocks and lanes run.
//
// Termination.  parent[i] <= i always holds, with equality exactly at roots, and entries only ever decrease.  A find
// follows parent only while it is strictly smaller than where it stands, so it ends after at most i + 1 steps whatever
// it reads; it then lowers the entry it started from to the ancestor it reached, which keeps all of this true.  A union
// repeats only when its atomicMin found parent[a] != a, that is after another lane installed a
// strictly smaller value there since our find; every such repeat is paid for by one strict decrease of one entry, and
// the entries are bounded below by 0.  Both loops carry a hard cap as well: a bug gives a wrong label, never a hang.
//
// component_pixel is a rank-select over the flattened label map: per 2048-pixel segment the count of label == root,
// then one block per sample walks the segment counts and selects inside the one segment that holds rank k.
#include "common.h"

namespace {

constexpr int kMaxSamples = 16;                  // records per launch, by value in the kernel argument
constexpr int kTile = 64;                        // tile edge of launch 1 (tests/test_components_gpu.py states it)
constexpr int kTilePix = kTile * kTile;
constexpr int kThreads = 256;
constexpr int kPerLane = 8;                      // pixels per lane of the linear launches (3, 5, rank-select)
constexpr int kChunk = kThreads * kPerLane;      // 2048 pixels per block

struct CcBatch { DcfpCcSample s[kMaxSamples]; };

// a sample's slice of the work buffer, in int32 units; every region starts on a 16-byte boundary
struct CcLayout {
    long long P, cap, nblk;
    long long parent, aux, roots, sizes, blk, seg, total;
};

__host__ __device__ inline long long up4(long long n) { return (n + 3) & ~3LL; }

__host__ __device__ inline CcLayout cc_layout(int Hp, int Wp) {
    CcLayout L;
    L.P = (long long)Hp * Wp;
    L.cap = (long long)((Hp + 1) / 2) * ((Wp + 1) / 2);      // most components 8-connectivity allows
    L.nblk = (L.P + kChunk - 1) / kChunk;
    const long long P8 = (L.P + 7) & ~7LL;
    L.parent = 0;
    L.aux = L.parent + P8;
    L.roots = L.aux + P8;
    L.sizes = L.roots + up4(L.cap);
    L.blk = L.sizes + up4(L.cap);
    L.seg = L.blk + up4(L.nblk);
    L.total = L.seg + up4(L.nblk);
    return L;
}

__device__ __forceinline__ int32_t* cc_slice(void* work, const DcfpCcSample& s) {
    return reinterpret_cast<int32_t*>(static_cast<char*>(work) + s.work_off);
}

// ---- union-find by minimum.  SCOPE: workgroup for the LDS forest of launch 1, agent for the global one of launch 2.
template <int SCOPE>
__device__ __forceinline__ int cc_find(int* parent, int a) {
    // strictly decreasing: at most a + 1 steps (header, "Termination")
    const int a0 = a;
    int first = -1;
    for (int it = 0; it <= 0x40000000; ++it) {
        const int p = __hip_atomic_load(&parent[a], __ATOMIC_RELAXED, SCOPE);
        if (it == 0) first = p;
        if (p >= a || p < 0) break;
        a = p;
    }
    // one-step compression: a is an ancestor of a0 below its parent, so the entry decreases and stays inside the set
    if (a < first) atomicMin(&parent[a0], a);
    return a;
}

template <int SCOPE>
__device__ __forceinline__ void cc_union(int* parent, int a, int b, int cap) {
    // repeats only after another lane lowered parent[a] (header, "Termination"); `cap` is the hard stop
    for (int it = 0; it < cap; ++it) {
        a = cc_find<SCOPE>(parent, a);
        b = cc_find<SCOPE>(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&parent[a], b);
        if (old == a) return;
        a = old;                                   // old < a: a was linked meanwhile; join that set with b's instead
    }
}

// exclusive scan over the 256 lanes of a block (eight fixed steps); *total = the sum
__device__ __forceinline__ int block_excl_scan(int v, int* sh, int* total) {
    const int t = (int)threadIdx.x;
    sh[t] = v;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < kThreads; off <<= 1) {
        const int a = t >= off ? sh[t - off] : 0;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    const int incl = sh[t];
    *total = sh[kThreads - 1];
    __syncthreads();
    return incl - v;
}

// ---- launch 1
__global__ __launch_bounds__(kThreads) void cc_tile_kernel(CcBatch batch, const int32_t* __restrict__ maps,
                                                          const uint8_t* __restrict__ id_table, void* work) {
    __shared__ int lab[kTilePix];
    __shared__ int cnt[kTilePix];
    __shared__ uint8_t sId[256];
    const DcfpCcSample& s = batch.s[blockIdx.y];
    const int Hp = s.Hp, Wp = s.Wp;
    const int tiles_x = (Wp + kTile - 1) / kTile, tiles_y = (Hp + kTile - 1) / kTile;
    if ((long long)blockIdx.x >= (long long)tiles_x * tiles_y) return;        // uniform over the block
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x % tiles_x;
    const int tid = (int)threadIdx.x;
    sId[tid] = id_table ? id_table[tid] : (uint8_t)tid;
    __syncthreads();

    const int32_t* row_map = maps + s.row_off;
    const int32_t* col_map = maps + s.col_off;
#pragma unroll 4
    for (int i = tid; i < kTilePix; i += kThreads) {
        const int y = ty * kTile + i / kTile, x = tx * kTile + i % kTile;
        bool fg = false;
        if (y < s.dst_h && x < s.dst_w) {
            const int sy = min(max(row_map[y], 0), s.src_h - 1), sx = min(max(col_map[x], 0), s.src_w - 1);
            fg = (int)sId[s.label[(long long)sy * s.src_w + sx]] == s.cls;
        }
        lab[i] = fg ? i : -1;
        cnt[i] = 0;
    }
    __syncthreads();

    // every 8-adjacent pair inside the tile is joined from its later pixel (W, NW, N, NE).  With N set, NW and NE are
    // N's own horizontal neighbours; with W set, NW is W's vertical neighbour: those unions are made there.
    for (int i = tid; i < kTilePix; i += kThreads) {
        if (lab[i] < 0) continue;                 // foreground entries never become negative
        const int ly = i / kTile, lx = i % kTile;
        const bool w = lx > 0 && lab[i - 1] >= 0;
        if (w) cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, i, i - 1, kTilePix);
        if (ly > 0) {
            if (lab[i - kTile] >= 0) {
                cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, i, i - kTile, kTilePix);
            } else {
                if (!w && lx > 0 && lab[i - kTile - 1] >= 0)
                    cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, i, i - kTile - 1, kTilePix);
                if (lx < kTile - 1 && lab[i - kTile + 1] >= 0)
                    cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, i, i - kTile + 1, kTilePix);
            }
        }
    }
    __syncthreads();

    int root[kTilePix / kThreads];
#pragma unroll
    for (int j = 0; j < kTilePix / kThreads; ++j) {
        const int i = tid + j * kThreads;
        root[j] = lab[i] < 0 ? -1 : cc_find<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, i);
        if (root[j] >= 0) atomicAdd(&cnt[root[j]], 1);
    }
    __syncthreads();

    const CcLayout L = cc_layout(Hp, Wp);
    int32_t* base = cc_slice(work, s);
    int32_t* parent = base + L.parent;
    int32_t* aux = base + L.aux;
#pragma unroll
    for (int j = 0; j < kTilePix / kThreads; ++j) {
        const int i = tid + j * kThreads;
        const int y = ty * kTile + i / kTile, x = tx * kTile + i % kTile;
        if (y >= Hp || x >= Wp) continue;
        const int r = root[j];
        const long long p = (long long)y * Wp + x;
        // local order (ly, lx) and linear order y*Wp + x agree inside a tile: the local minimum is the global one
        parent[p] = r < 0 ? -1 : (ty * kTile + r / kTile) * Wp + tx * kTile + r % kTile;
        aux[p] = r == i ? cnt[i] : 0;
    }
}

// ---- launch 2
__global__ __launch_bounds__(kThreads) void cc_merge_kernel(CcBatch batch, void* work) {
    const DcfpCcSample& s = batch.s[blockIdx.y];
    const int Hp = s.Hp, Wp = s.Wp;
    const int tiles_x = (Wp + kTile - 1) / kTile, tiles_y = (Hp + kTile - 1) / kTile;
    const long long nH = (long long)(tiles_y - 1) * Wp, nV = (long long)(tiles_x - 1) * Hp;
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= nH + nV) return;
    int32_t* parent = cc_slice(work, s) + cc_layout(Hp, Wp).parent;
    const int cap = (int)((long long)Hp * Wp);
    int y, x, qy[3], qx[3];
    if (i < nH) {                                  // first row of a tile: the three neighbours above the line
        y = ((int)(i / Wp) + 1) * kTile;
        x = (int)(i % Wp);
        for (int j = 0; j < 3; ++j) { qy[j] = y - 1; qx[j] = x - 1 + j; }
    } else {                                       // first column of a tile: the three neighbours left of the line
        const long long v = i - nH;
        x = ((int)(v / Hp) + 1) * kTile;
        y = (int)(v % Hp);
        for (int j = 0; j < 3; ++j) { qy[j] = y - 1 + j; qx[j] = x - 1; }
    }
    const int p = y * Wp + x;
    if (__hip_atomic_load(&parent[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) return;
    for (int j = 0; j < 3; ++j) {
        if (qy[j] < 0 || qy[j] >= Hp || qx[j] < 0 || qx[j] >= Wp) continue;
        const int q = qy[j] * Wp + qx[j];
        if (__hip_atomic_load(&parent[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) continue;
        cc_union<__HIP_MEMORY_SCOPE_AGENT>(parent, p, q, cap);
    }
}

// The forest is final here: launch 3 only replaces entries by their root, so a find that meets a value another block
// has already replaced still walks to the same root.  Plain loads.
__device__ __forceinline__ int cc_find_plain(const int32_t* parent, int a) {
    for (int it = 0; it <= 0x40000000; ++it) {     // strictly decreasing: at most a + 1 steps
        const int p = parent[a];
        if (p >= a || p < 0) break;
        a = p;
    }
    return a;
}

__device__ __forceinline__ void cc_load8(const int32_t* a, long long p0, long long P, int v[kPerLane]) {
    if (p0 + kPerLane <= P) {
        const int4 lo = *reinterpret_cast<const int4*>(a + p0), hi = *reinterpret_cast<const int4*>(a + p0 + 4);
        v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
        v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
    } else {
#pragma unroll
        for (int j = 0; j < kPerLane; ++j) v[j] = p0 + j < P ? a[p0 + j] : -1;
    }
}

// ---- launch 3
__global__ __launch_bounds__(kThreads) void cc_flatten_kernel(CcBatch batch, void* work) {
    __shared__ int sh[kThreads];
    const DcfpCcSample& s = batch.s[blockIdx.y];
    const CcLayout L = cc_layout(s.Hp, s.Wp);
    if ((long long)blockIdx.x >= L.nblk) return;
    int32_t* base = cc_slice(work, s);
    int32_t* parent = base + L.parent;
    int32_t* aux = base + L.aux;
    const long long p0 = (long long)blockIdx.x * kChunk + (long long)threadIdx.x * kPerLane;
    int v[kPerLane], roots = 0;
    cc_load8(parent, p0, L.P, v);
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
        if (v[j] < 0) continue;
        const int p = (int)(p0 + j);
        const int r = cc_find_plain(parent, v[j]);
        roots += r == p;
        if (r != p) {
            if (r != v[j]) parent[p] = r;
            const int c = aux[p];                 // > 0 only at the root of a tile-local component; nobody adds there
            if (c > 0) atomicAdd(&aux[r], c);
        }
    }
    int total;
    block_excl_scan(roots, sh, &total);
    if (threadIdx.x == 0) base[L.blk + blockIdx.x] = total;
}

// ---- launch 4
__global__ __launch_bounds__(kThreads) void cc_scan_kernel(CcBatch batch, void* work, int n0, int32_t* counts) {
    __shared__ int sh[kThreads];
    const DcfpCcSample& s = batch.s[blockIdx.x];
    const CcLayout L = cc_layout(s.Hp, s.Wp);
    int32_t* blk = cc_slice(work, s) + L.blk;
    int carry = 0;
    for (long long b0 = 0; b0 < L.nblk; b0 += kThreads) {      // ceil(nblk / 256) rounds
        const long long b = b0 + threadIdx.x;
        const int c = b < L.nblk ? blk[b] : 0;
        int total;
        const int ex = block_excl_scan(c, sh, &total);
        if (b < L.nblk) blk[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) counts[n0 + blockIdx.x] = carry;
}

// ---- launch 5
__global__ __launch_bounds__(kThreads) void cc_compact_kernel(CcBatch batch, void* work) {
    __shared__ int sh[kThreads];
    const DcfpCcSample& s = batch.s[blockIdx.y];
    const CcLayout L = cc_layout(s.Hp, s.Wp);
    if ((long long)blockIdx.x >= L.nblk) return;
    int32_t* base = cc_slice(work, s);
    const int32_t* label = base + L.parent;
    const long long p0 = (long long)blockIdx.x * kChunk + (long long)threadIdx.x * kPerLane;
    int v[kPerLane], roots = 0;
    cc_load8(label, p0, L.P, v);
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) roots += v[j] >= 0 && v[j] == p0 + j;
    int total;
    long long at = base[L.blk + blockIdx.x] + block_excl_scan(roots, sh, &total);
    if (!roots) return;
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
        if (v[j] < 0 || v[j] != p0 + j) continue;
        if (at < L.cap) {                          // holds by the 8-connectivity bound; kept as the bounds check
            base[L.roots + at] = v[j];
            base[L.sizes + at] = base[L.aux + v[j]];
        }
        ++at;
    }
}

// ---- rank-select, pass A: per segment, the number of pixels of the chosen component
__global__ __launch_bounds__(kThreads) void cc_segcount_kernel(CcBatch batch, void* work, int n0,
                                                              const int32_t* __restrict__ counts,
                                                              const int32_t* __restrict__ sel_n) {
    __shared__ int sh[kThreads];
    const DcfpCcSample& s = batch.s[blockIdx.y];
    const CcLayout L = cc_layout(s.Hp, s.Wp);
    const int n = sel_n[n0 + blockIdx.y];
    if ((long long)blockIdx.x >= L.nblk || n < 1 || n > counts[n0 + blockIdx.y] || n > L.cap) return;
    int32_t* base = cc_slice(work, s);
    const int root = base[L.roots + n - 1];
    const long long p0 = (long long)blockIdx.x * kChunk + (long long)threadIdx.x * kPerLane;
    int v[kPerLane], c = 0;
    cc_load8(base + L.parent, p0, L.P, v);
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) c += v[j] == root;
    int total;
    block_excl_scan(c, sh, &total);
    if (threadIdx.x == 0) base[L.seg + blockIdx.x] = total;
}

// ---- rank-select, pass B: one block per sample finds the segment that holds rank k, then the pixel inside it
__global__ __launch_bounds__(kThreads) void cc_select_kernel(CcBatch batch, void* work, int n0,
                                                            const int32_t* __restrict__ counts,
                                                            const int32_t* __restrict__ sel_n,
                                                            const int32_t* __restrict__ sel_k, int32_t* yx) {
    __shared__ int sh[kThreads];
    __shared__ long long hit_seg;
    __shared__ int hit_rank;
    const DcfpCcSample& s = batch.s[blockIdx.x];
    const CcLayout L = cc_layout(s.Hp, s.Wp);
    const int at = n0 + (int)blockIdx.x;
    const int n = sel_n[at], k = sel_k[at];
    int32_t* out = yx + 2LL * at;
    if (threadIdx.x == 0) {
        out[0] = out[1] = -1;
        hit_seg = -1;
        hit_rank = 0;
    }
    if (n < 1 || n > counts[at] || n > L.cap || k < 0) return;                 // uniform over the block
    __syncthreads();
    int32_t* base = cc_slice(work, s);
    const int root = base[L.roots + n - 1];
    int carry = 0;
    for (long long b0 = 0; b0 < L.nblk; b0 += kThreads) {      // ceil(nblk / 256) rounds, ended early at the hit
        const long long b = b0 + threadIdx.x;
        const int c = b < L.nblk ? base[L.seg + b] : 0;
        int total;
        const int ex = carry + block_excl_scan(c, sh, &total);
        if (c > 0 && ex <= k && k < ex + c) {     // at most one lane: the segments' rank ranges are disjoint
            hit_seg = b;
            hit_rank = k - ex;
        }
        carry += total;
        __syncthreads();
        if (hit_seg >= 0 || carry > k) break;
    }
    if (hit_seg < 0) return;                       // k >= size of the component
    const long long p0 = hit_seg * kChunk + (long long)threadIdx.x * kPerLane;
    const int rank = hit_rank;
    int v[kPerLane], c = 0;
    cc_load8(base + L.parent, p0, L.P, v);
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) c += v[j] == root;
    int total;
    int ex = block_excl_scan(c, sh, &total);
    if (c > 0 && ex <= rank && rank < ex + c) {
#pragma unroll
        for (int j = 0; j < kPerLane; ++j) {
            if (v[j] != root) continue;
            if (ex == rank) {
                const long long p = p0 + j;
                out[0] = (int)(p / s.Wp);
                out[1] = (int)(p % s.Wp);
            }
            ++ex;
        }
    }
}

bool cc_valid(const DcfpCcSample* samples, int N, int64_t n_maps, size_t work_bytes, bool need_label) {
    for (int i = 0; i < N; ++i) {
        const DcfpCcSample& s = samples[i];
        if ((need_label && !s.label) || s.src_h <= 0 || s.src_w <= 0 || (long long)s.src_h * s.src_w > 0x7fffffffLL ||
            s.dst_h <= 0 || s.dst_w <= 0 || s.Hp < s.dst_h || s.Wp < s.dst_w || (long long)s.Hp * s.Wp > (1LL << 30) ||
            s.cls < 0 || s.cls > 255 || s.work_off < 0 || (s.work_off & 15))
            return false;
        if (need_label && (s.row_off < 0 || (long long)s.row_off + s.dst_h > n_maps || s.col_off < 0 ||
                           (long long)s.col_off + s.dst_w > n_maps))
            return false;
        const unsigned long long need = (unsigned long long)cc_layout(s.Hp, s.Wp).total * sizeof(int32_t);
        if ((unsigned long long)s.work_off > work_bytes || need > work_bytes - (unsigned long long)s.work_off) return false;
    }
    return true;
}

}  // namespace

extern "C" size_t dcfp_components_workspace_bytes(int Hp, int Wp) {
    if (Hp <= 0 || Wp <= 0 || (long long)Hp * Wp > (1LL << 30)) return 0;
    return (size_t)cc_layout(Hp, Wp).total * sizeof(int32_t);
}

extern "C" int dcfp_label_components_u8(const DcfpCcSample* samples, int N, const int32_t* maps, int64_t n_maps,
                                        const uint8_t* id_table, void* work, size_t work_bytes, int32_t* counts,
                                        dcfp_stream_t stream) {
    if (!samples || N <= 0 || !maps || n_maps <= 0 || !work || !counts || !dcfp_aligned16(work) ||
        (reinterpret_cast<uintptr_t>(maps) & 3u) || (reinterpret_cast<uintptr_t>(counts) & 3u))
        return DCFP_E_BADDESC;
    if (!cc_valid(samples, N, n_maps, work_bytes, true)) return DCFP_E_BADDESC;
    for (int n0 = 0; n0 < N; n0 += kMaxSamples) {
        const int cnt = N - n0 < kMaxSamples ? N - n0 : kMaxSamples;
        CcBatch batch;
        long long tiles = 1, border = 0, nblk = 1;
        for (int i = 0; i < kMaxSamples; ++i) {
            const DcfpCcSample& s = batch.s[i] = samples[n0 + (i < cnt ? i : 0)];
            const long long tx = (s.Wp + kTile - 1) / kTile, ty = (s.Hp + kTile - 1) / kTile;
            const long long b = (ty - 1) * s.Wp + (tx - 1) * s.Hp, nb = cc_layout(s.Hp, s.Wp).nblk;
            tiles = tx * ty > tiles ? tx * ty : tiles;
            border = b > border ? b : border;
            nblk = nb > nblk ? nb : nblk;
        }
        hipStream_t st = dcfp_s(stream);
        hipLaunchKernelGGL(cc_tile_kernel, dim3((unsigned)tiles, (unsigned)cnt), dim3(kThreads), 0, st, batch, maps,
                           id_table, work);
        if (border > 0)
            hipLaunchKernelGGL(cc_merge_kernel, dim3((unsigned)((border + kThreads - 1) / kThreads), (unsigned)cnt),
                               dim3(kThreads), 0, st, batch, work);
        hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)nblk, (unsigned)cnt), dim3(kThreads), 0, st, batch, work);
        hipLaunchKernelGGL(cc_scan_kernel, dim3((unsigned)cnt), dim3(kThreads), 0, st, batch, work, n0, counts);
        hipLaunchKernelGGL(cc_compact_kernel, dim3((unsigned)nblk, (unsigned)cnt), dim3(kThreads), 0, st, batch, work);
    }
    DCFP_RETURN_LAUNCH();
}

extern "C" int dcfp_component_pixel_i32(const DcfpCcSample* samples, int N, void* work, size_t work_bytes,
                                        const int32_t* counts, const int32_t* n, const int32_t* k, int32_t* yx,
                                        dcfp_stream_t stream) {
    if (!samples || N <= 0 || !work || !counts || !n || !k || !yx || !dcfp_aligned16(work) ||
        ((reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(n) | reinterpret_cast<uintptr_t>(k) |
          reinterpret_cast<uintptr_t>(yx)) & 3u))
        return DCFP_E_BADDESC;
    if (!cc_valid(samples, N, 0, work_bytes, false)) return DCFP_E_BADDESC;
    for (int n0 = 0; n0 < N; n0 += kMaxSamples) {
        const int cnt = N - n0 < kMaxSamples ? N - n0 : kMaxSamples;
        CcBatch batch;
        long long nblk = 1;
        for (int i = 0; i < kMaxSamples; ++i) {
            const DcfpCcSample& s = batch.s[i] = samples[n0 + (i < cnt ? i : 0)];
            const long long nb = cc_layout(s.Hp, s.Wp).nblk;
            nblk = nb > nblk ? nb : nblk;
        }
        hipStream_t st = dcfp_s(stream);
        hipLaunchKernelGGL(cc_segcount_kernel, dim3((unsigned)nblk, (unsigned)cnt), dim3(kThreads), 0, st, batch, work,
                           n0, counts, n);
        hipLaunchKernelGGL(cc_select_kernel, dim3((unsigned)cnt), dim3(kThreads), 0, st, batch, work, n0, counts, n, k,
                           yx);
    }
    DCFP_RETURN_LAUNCH();
}
