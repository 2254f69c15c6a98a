// ppm.hip — the pyramid pooling module of PSPNet (networks/tools/ppm.py): adaptive average pooling to up to four
// small grids, and the two adjoints of its backward.  Fixed summation orders, no atomics: every run gives the same bits.
//
// Pool + place (ppm_pool_kernel): one block per (n, c) plane streams it once, in chunks of rows staged in LDS, and
//   optionally copies each chunk into a channel slice of a batch-strided, row-pitched destination (the concat buffer).
//   PyTorch's windows (start = floor(i*H/s), end = ceil((i+1)*H/s)) overlap when s does not divide H, so the plane is
//   summed into "atoms": the cells between all the levels' window boundaries, rows and columns.  A chunk's rows are
//   first reduced over each column atom (X ascending), then added into the atoms (Y ascending); every bin of every
//   level is then a sum of atoms (row atom ascending, then column atom ascending), divided by its area for a mean.
//
// Pool adjoint (ppm_pool_adjoint_kernel): dx = g + sum over levels (as given), bins i ascending, j ascending of
//   dp[bin] / area[bin] over the bins whose window holds (y, x); g (the layer4 slice of the concat gradient, dense or
//   row-pitched) may be absent.  g is read once and dx written once.
//
// Bilinear adjoint onto small grids (ppm_resize_adjoint_kernel): dp[i, j] = sum_Y wy(Y, i) * sum_X wx(X, j) * g[Y, X]
//   (Y ascending, X ascending) with the index math of bilinear.h, for s x s targets (s <= 8).  One block per (n, channel
//   of the concatenated prior slices): the level follows from the channel.  All lanes stream the plane: chunks of rows
//   staged in LDS, the column reduction split over the lanes in fixed parts, then one lane per dp cell adds the rows.
#include "common.h"
#include "bilinear.h"

namespace {

using namespace dcfp_bilinear;

constexpr int kThreads = 256;
constexpr int kMaxLevels = 4;
constexpr int kMaxS = 8;
constexpr int kMaxCuts = 2 * kMaxLevels * kMaxS + 2;   // window boundaries along one axis (atoms: one fewer)
constexpr int kStageFloats = 4096;                     // LDS floats of staged rows per chunk
constexpr int kMaxChunkRows = 32;
constexpr int kAdjRows = 16;                           // dx rows per pool-adjoint block
constexpr int kMaxResizeW = 2048;                      // LDS bound of the per-column taps of the resize adjoint

struct PoolGeom {
    int nlev;
    int sh[kMaxLevels], sw[kMaxLevels];
    long long off[kMaxLevels];                          // element offset of level l's [N, C, sh, sw] block
    int nra, nca;                                       // row / column atoms
    int rcut[kMaxCuts], ccut[kMaxCuts];                 // atom a: rows [rcut[a], rcut[a + 1])
    int ra[kMaxLevels][kMaxS][2], ca[kMaxLevels][kMaxS][2];   // atoms [lo, hi) of the window of bin row i / column j
};

struct ResizeGeom {
    int nlev;
    int sh[kMaxLevels], sw[kMaxLevels];
    int cbeg[kMaxLevels + 1];                           // channel offsets of the levels in the prior slices
    long long off[kMaxLevels];                          // element offset of level l's [N, C_l, sh, sw] block in dp
    float scale_h[kMaxLevels], scale_w[kMaxLevels];     // bilinear.h host_scale(s, H / W, align_corners)
};

template <int VEC>
struct Vec;
template <>
struct Vec<1> {
    using T = float;
    __device__ static float get(const T& v, int) { return v; }
    __device__ static void set(T& v, int, float f) { v = f; }
};
template <>
struct Vec<4> {
    using T = float4;
    __device__ static float get(const T& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }
    __device__ static void set(T& v, int k, float f) {
        if (k == 0) v.x = f; else if (k == 1) v.y = f; else if (k == 2) v.z = f; else v.w = f;
    }
};

// ------------------------------------------------------------------------------------------------ pool + place
template <int VEC>
__global__ void __launch_bounds__(kThreads)
ppm_pool_kernel(const float* __restrict__ x, int C, int H, int W, float* __restrict__ out, int mean,
                float* __restrict__ dst, long long dst_nstride, int dst_pitch, int R, const PoolGeom G) {
    using V = typename Vec<VEC>::T;
    extern __shared__ float smem[];
    float* stage = smem;                                // R * W
    float* rp = stage + R * W;                          // R * nca
    float* atoms = rp + R * G.nca;                      // nra * nca
    const long long plane = blockIdx.x;
    const int n = (int)(plane / C), c = (int)(plane - (long long)n * C);
    const float* p = x + plane * H * W;
    float* q = dst ? dst + (long long)n * dst_nstride + (long long)c * H * dst_pitch : nullptr;
    const int nca = G.nca, natoms = G.nra * G.nca;
    for (int t = threadIdx.x; t < natoms; t += kThreads) atoms[t] = 0.f;
    const int wv = W / VEC;

    for (int y0 = 0; y0 < H; y0 += R) {
        const int rows = min(R, H - y0);
        __syncthreads();                                // the previous chunk's rows and partials are consumed
        for (int e = threadIdx.x; e < rows * wv; e += kThreads) {
            const int r = e / wv, xv = e - r * wv;
            const V v = reinterpret_cast<const V*>(p + (long long)(y0 + r) * W)[xv];
            reinterpret_cast<V*>(stage + r * W)[xv] = v;
            if (q) reinterpret_cast<V*>(q + (long long)(y0 + r) * dst_pitch)[xv] = v;
        }
        __syncthreads();
        for (int t = threadIdx.x; t < rows * nca; t += kThreads) {     // row partials over the column atoms
            const int r = t / nca, a = t - r * nca;
            const float* s = stage + r * W;
            float acc = 0.f;
            for (int X = G.ccut[a]; X < G.ccut[a + 1]; ++X) acc += s[X];
            rp[t] = acc;
        }
        __syncthreads();
        for (int t = threadIdx.x; t < natoms; t += kThreads) {         // each atom owned by one lane: rows ascending
            const int ra = t / nca, a = t - ra * nca;
            const int ya = max(G.rcut[ra], y0), yb = min(G.rcut[ra + 1], y0 + rows);
            float acc = atoms[t];
            for (int y = ya; y < yb; ++y) acc += rp[(y - y0) * nca + a];
            atoms[t] = acc;
        }
    }
    __syncthreads();
    int nb = 0;
    for (int l = 0; l < G.nlev; ++l) nb += G.sh[l] * G.sw[l];
    for (int t = threadIdx.x; t < nb; t += kThreads) {
        int l = 0, b = t;
        while (b >= G.sh[l] * G.sw[l]) { b -= G.sh[l] * G.sw[l]; ++l; }
        const int i = b / G.sw[l], j = b - i * G.sw[l];
        const int r0 = G.ra[l][i][0], r1 = G.ra[l][i][1], c0 = G.ca[l][j][0], c1 = G.ca[l][j][1];
        float acc = 0.f;
        for (int ra = r0; ra < r1; ++ra)
            for (int a = c0; a < c1; ++a) acc += atoms[ra * nca + a];
        if (mean) acc /= (float)((G.rcut[r1] - G.rcut[r0]) * (G.ccut[c1] - G.ccut[c0]));
        out[G.off[l] + plane * G.sh[l] * G.sw[l] + b] = acc;
    }
}

// ---------------------------------------------------------------------------------------------- pool adjoint
template <int VEC>
__global__ void __launch_bounds__(kThreads)
ppm_pool_adjoint_kernel(const float* __restrict__ dp, int C, int H, int W, const float* __restrict__ g,
                        long long g_nstride, int g_pitch, float* __restrict__ dx, const PoolGeom G) {
    using V = typename Vec<VEC>::T;
    __shared__ float qv[kMaxLevels * kMaxS * kMaxS];    // dp / area of this plane's bins, level-major
    __shared__ int rb[kAdjRows * kMaxLevels];           // bin rows [lo, hi] holding each row of the band
    const long long plane = blockIdx.x;
    const int n = (int)(plane / C), c = (int)(plane - (long long)n * C);
    int qoff[kMaxLevels];
    int nb = 0;
#pragma unroll
    for (int l = 0; l < kMaxLevels; ++l) { qoff[l] = nb; if (l < G.nlev) nb += G.sh[l] * G.sw[l]; }
    for (int t = threadIdx.x; t < nb; t += kThreads) {
        int l = 0, b = t;
        while (b >= G.sh[l] * G.sw[l]) { b -= G.sh[l] * G.sw[l]; ++l; }
        const int i = b / G.sw[l], j = b - i * G.sw[l];
        const int r0 = G.ra[l][i][0], r1 = G.ra[l][i][1], c0 = G.ca[l][j][0], c1 = G.ca[l][j][1];
        const float area = (float)((G.rcut[r1] - G.rcut[r0]) * (G.ccut[c1] - G.ccut[c0]));
        qv[t] = dp[G.off[l] + plane * G.sh[l] * G.sw[l] + b] / area;
    }
    const int y0 = blockIdx.y * kAdjRows;
    const int rows = min(kAdjRows, H - y0);
    for (int t = threadIdx.x; t < rows * G.nlev; t += kThreads) {
        const int r = t / G.nlev, l = t - r * G.nlev, y = y0 + r;
        int lo = kMaxS, hi = -1;
        for (int i = 0; i < G.sh[l]; ++i)
            if (G.rcut[G.ra[l][i][0]] <= y && y < G.rcut[G.ra[l][i][1]]) { lo = min(lo, i); hi = i; }
        rb[t] = lo | (hi << 8);
    }
    __syncthreads();
    const float* gp = g ? g + (long long)n * g_nstride + (long long)c * H * g_pitch : nullptr;
    float* o = dx + plane * H * W;
    const int wv = W / VEC;
    for (int xv = threadIdx.x; xv < wv; xv += kThreads) {
        int jl[VEC][kMaxLevels], jh[VEC][kMaxLevels];   // bin columns [lo, hi] holding each of this lane's columns
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const int X = xv * VEC + k;
#pragma unroll
            for (int l = 0; l < kMaxLevels; ++l) {
                int lo = kMaxS, hi = -1;
                if (l < G.nlev)
                    for (int j = 0; j < G.sw[l]; ++j)
                        if (G.ccut[G.ca[l][j][0]] <= X && X < G.ccut[G.ca[l][j][1]]) { lo = min(lo, j); hi = j; }
                jl[k][l] = lo; jh[k][l] = hi;
            }
        }
        for (int r = 0; r < rows; ++r) {
            const int y = y0 + r;
            V v;
            if (gp) v = reinterpret_cast<const V*>(gp + (long long)y * g_pitch)[xv];
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                float acc = gp ? Vec<VEC>::get(v, k) : 0.f;
#pragma unroll
                for (int l = 0; l < kMaxLevels; ++l) {       // (constant bounds: jl / jh stay in registers)
                    if (l >= G.nlev) break;
                    const int e = rb[r * G.nlev + l];
                    const int il = e & 255, ih = e >> 8;
                    for (int i = il; i <= ih; ++i)
                        for (int j = jl[k][l]; j <= jh[k][l]; ++j) acc += qv[qoff[l] + i * G.sw[l] + j];
                }
                Vec<VEC>::set(v, k, acc);
            }
            reinterpret_cast<V*>(o + (long long)y * W)[xv] = v;
        }
    }
}

// ------------------------------------------------------------------------------- bilinear adjoint, small grids
template <bool ALIGN, int VEC>
__global__ void __launch_bounds__(kThreads)
ppm_resize_adjoint_kernel(const float* __restrict__ g, long long g_nstride, int g_pitch, int H, int W,
                          float* __restrict__ dp, int R, const ResizeGeom G) {
    using V = typename Vec<VEC>::T;
    extern __shared__ float smem[];
    float* stage = smem;                                // R * W
    float* w0 = stage + R * W;                          // W: weight of column X onto j0[X]
    float* w1 = w0 + W;                                 // W: weight of column X onto j0[X] + 1
    int* j0 = reinterpret_cast<int*>(w1 + W);           // W
    float* part = reinterpret_cast<float*>(j0 + W);     // parts of the column reductions: <= kThreads
    __shared__ int xr[kMaxS][2];                        // columns [lo, hi] with a tap on target column j
    const int cc = blockIdx.x, n = blockIdx.y;
    int l = 0;
    while (l + 1 < G.nlev && cc >= G.cbeg[l + 1]) ++l;
    const int Cl = G.cbeg[l + 1] - G.cbeg[l], c = cc - G.cbeg[l];
    const int sh = G.sh[l], sw = G.sw[l];
    const float* p = g + (long long)n * g_nstride + (long long)cc * H * g_pitch;

    for (int j = threadIdx.x; j < kMaxS; j += kThreads) { xr[j][0] = W; xr[j][1] = -1; }
    for (int X = threadIdx.x; X < W; X += kThreads) {
        const Lerp L = lerp_of<ALIGN>(X, G.scale_w[l], sw);
        j0[X] = L.i0;
        w0[X] = tap_weight(L, L.i0);
        w1[X] = L.i1 != L.i0 ? tap_weight(L, L.i1) : 0.f;
    }
    __syncthreads();
    // (j0 is non-decreasing in X: the columns with a tap on j are those with j - 1 <= j0[X] <= j, one run)
    for (int X = threadIdx.x; X < W; X += kThreads) {
        const int a = X > 0 ? j0[X - 1] : -2, b = j0[X];
        for (int j = max(a + 2, 0); j <= min(b + 1, sw - 1); ++j) xr[j][0] = X;
        const int e = X + 1 < W ? j0[X + 1] : sw + 1;
        for (int j = max(b, 0); j <= min(e - 1, sw - 1); ++j) xr[j][1] = X;
    }
    // the column reduction of a chunk: rows * sw * P tasks, a target column's run of X split in P fixed parts
    const int P = max(1, kThreads / (R * sw));
    const int wv = W / VEC;
    float acc = 0.f;                                    // lane t < sh * sw: dp[t / sw, t % sw]
    const int ti = threadIdx.x / sw, tj = threadIdx.x - ti * sw;
    for (int y0 = 0; y0 < H; y0 += R) {
        const int rows = min(R, H - y0);
        __syncthreads();                                // (also orders xr / the taps before their first use)
        for (int e = threadIdx.x; e < rows * wv; e += kThreads) {
            const int r = e / wv, xv = e - r * wv;
            reinterpret_cast<V*>(stage + r * W)[xv] = reinterpret_cast<const V*>(p + (long long)(y0 + r) * g_pitch)[xv];
        }
        __syncthreads();
        for (int t = threadIdx.x; t < rows * sw * P; t += kThreads) {
            const int r = t / (sw * P), rest = t - r * sw * P, j = rest / P, k = rest - j * P;
            const int lo = xr[j][0], len = xr[j][1] - lo + 1;
            const int a = lo + (len > 0 ? len * k / P : 0), b = lo + (len > 0 ? len * (k + 1) / P : 0);
            const float* s = stage + r * W;
            float v = 0.f;
            for (int X = a; X < b; ++X) {
                const float wt = (j0[X] == j ? w0[X] : 0.f) + (j0[X] + 1 == j ? w1[X] : 0.f);
                if (wt != 0.f) v += wt * s[X];
            }
            part[t] = v;
        }
        __syncthreads();
        if (threadIdx.x < sh * sw) {
            for (int r = 0; r < rows; ++r) {
                const float wy = tap_weight(lerp_of<ALIGN>(y0 + r, G.scale_h[l], sh), ti);
                if (wy == 0.f) continue;
                float v = 0.f;
                for (int k = 0; k < P; ++k) v += part[(r * sw + tj) * P + k];
                acc += wy * v;
            }
        }
    }
    if (threadIdx.x < sh * sw) dp[G.off[l] + (((long long)n * Cl + c) * sh + ti) * sw + tj] = acc;
}

// ----------------------------------------------------------------------------------------------------- host
// PyTorch's adaptive-pool windows of every level along one axis, as atoms: false if a size is out of range
bool axis_atoms(int len, int nlev, const int* s, int* cut, int& ncut, int (*bins)[kMaxS][2]) {
    int pts[kMaxCuts];
    int np = 0;
    for (int l = 0; l < nlev; ++l) {
        if (s[l] < 1 || s[l] > kMaxS) return false;
        for (int i = 0; i < s[l]; ++i) {
            pts[np++] = (int)(((long long)i * len) / s[l]);
            pts[np++] = (int)(((long long)(i + 1) * len + s[l] - 1) / s[l]);
        }
    }
    for (int a = 1; a < np; ++a)                        // insertion sort, then unique
        for (int b = a; b > 0 && pts[b - 1] > pts[b]; --b) { const int t = pts[b]; pts[b] = pts[b - 1]; pts[b - 1] = t; }
    ncut = 0;
    for (int a = 0; a < np; ++a)
        if (ncut == 0 || cut[ncut - 1] != pts[a]) cut[ncut++] = pts[a];
    for (int l = 0; l < nlev; ++l)
        for (int i = 0; i < s[l]; ++i) {
            const int st = (int)(((long long)i * len) / s[l]), en = (int)(((long long)(i + 1) * len + s[l] - 1) / s[l]);
            int lo = 0, hi = 0;
            for (int a = 0; a < ncut; ++a) {
                if (cut[a] == st) lo = a;
                if (cut[a] == en) hi = a;
            }
            bins[l][i][0] = lo;
            bins[l][i][1] = hi;
        }
    return true;
}

int pool_geom(int N, int C, int H, int W, int nlev, const int* level_hw, PoolGeom& G) {
    if (nlev < 1 || nlev > kMaxLevels || !level_hw) return DCFP_E_BADDESC;
    G = PoolGeom{};
    G.nlev = nlev;
    long long off = 0;
    for (int l = 0; l < nlev; ++l) {
        G.sh[l] = level_hw[2 * l];
        G.sw[l] = level_hw[2 * l + 1];
        if (G.sh[l] < 1 || G.sh[l] > kMaxS || G.sw[l] < 1 || G.sw[l] > kMaxS) return DCFP_E_UNSUPPORTED;
        G.off[l] = off;
        off += (long long)N * C * G.sh[l] * G.sw[l];
    }
    int ncut = 0;
    if (!axis_atoms(H, nlev, G.sh, G.rcut, ncut, G.ra)) return DCFP_E_UNSUPPORTED;
    G.nra = ncut - 1;
    if (!axis_atoms(W, nlev, G.sw, G.ccut, ncut, G.ca)) return DCFP_E_UNSUPPORTED;
    G.nca = ncut - 1;
    return DCFP_OK;
}

}  // namespace

extern "C" int dcfp_ppm_pool_f32(const float* x, int N, int C, int H, int W, int nlev, const int* level_hw,
                                 float* out, int mean, float* dst, int64_t dst_nstride, int dst_pitch,
                                 dcfp_stream_t stream) {
    if (!x || !out || N <= 0 || C <= 0 || H <= 0 || W <= 0) return DCFP_E_BADDESC;
    if (W > kStageFloats || (long long)N * C > 2147483647LL) return DCFP_E_UNSUPPORTED;
    PoolGeom G;
    const int st = pool_geom(N, C, H, W, nlev, level_hw, G);
    if (st != DCFP_OK) return st;
    const int pitch = dst_pitch ? dst_pitch : W;
    if (dst) {
        if (pitch < W) return DCFP_E_BADDESC;
        if (dst_nstride == 0) dst_nstride = (int64_t)C * H * pitch;
        if (dst_nstride < (int64_t)C * H * pitch) return DCFP_E_BADDESC;
    }
    int R = kStageFloats / W;
    R = R < 1 ? 1 : (R > kMaxChunkRows ? kMaxChunkRows : R);
    const size_t lds = sizeof(float) * ((size_t)R * W + (size_t)R * G.nca + (size_t)G.nra * G.nca);
    const bool v4 = W % 4 == 0 && dcfp_aligned16(x) &&
                    (!dst || (pitch % 4 == 0 && dst_nstride % 4 == 0 && dcfp_aligned16(dst)));
    const dim3 grid((unsigned)((long long)N * C));
    if (v4)
        hipLaunchKernelGGL(ppm_pool_kernel<4>, grid, dim3(kThreads), lds, dcfp_s(stream), x, C, H, W, out, mean, dst,
                           (long long)dst_nstride, pitch, R, G);
    else
        hipLaunchKernelGGL(ppm_pool_kernel<1>, grid, dim3(kThreads), lds, dcfp_s(stream), x, C, H, W, out, mean, dst,
                           (long long)dst_nstride, pitch, R, G);
    DCFP_RETURN_LAUNCH();
}

extern "C" int dcfp_ppm_pool_adjoint_f32(const float* dp, int N, int C, int H, int W, int nlev, const int* level_hw,
                                         const float* g, int64_t g_nstride, int g_pitch, float* dx,
                                         dcfp_stream_t stream) {
    if (!dp || !dx || N <= 0 || C <= 0 || H <= 0 || W <= 0) return DCFP_E_BADDESC;
    if ((long long)N * C > 2147483647LL || (H + kAdjRows - 1) / kAdjRows > 65535) return DCFP_E_UNSUPPORTED;
    PoolGeom G;
    const int st = pool_geom(N, C, H, W, nlev, level_hw, G);
    if (st != DCFP_OK) return st;
    const int pitch = g_pitch ? g_pitch : W;
    if (g) {
        if (pitch < W) return DCFP_E_BADDESC;
        if (g_nstride == 0) g_nstride = (int64_t)C * H * pitch;
        if (g_nstride < (int64_t)C * H * pitch) return DCFP_E_BADDESC;
    }
    const bool v4 = W % 4 == 0 && dcfp_aligned16(dx) &&
                    (!g || (pitch % 4 == 0 && g_nstride % 4 == 0 && dcfp_aligned16(g)));
    const dim3 grid((unsigned)((long long)N * C), (H + kAdjRows - 1) / kAdjRows);
    if (v4)
        hipLaunchKernelGGL(ppm_pool_adjoint_kernel<4>, grid, dim3(kThreads), 0, dcfp_s(stream), dp, C, H, W, g,
                           (long long)g_nstride, pitch, dx, G);
    else
        hipLaunchKernelGGL(ppm_pool_adjoint_kernel<1>, grid, dim3(kThreads), 0, dcfp_s(stream), dp, C, H, W, g,
                           (long long)g_nstride, pitch, dx, G);
    DCFP_RETURN_LAUNCH();
}

extern "C" int dcfp_ppm_resize_adjoint_f32(const float* g, int64_t g_nstride, int g_pitch, int N, int H, int W,
                                           int nlev, const int* level_chw, float* dp, int align_corners,
                                           dcfp_stream_t stream) {
    if (!g || !dp || !level_chw || N <= 0 || H <= 0 || W <= 0) return DCFP_E_BADDESC;
    if (nlev < 1 || nlev > kMaxLevels) return DCFP_E_BADDESC;
    if (W > kMaxResizeW || N > 65535) return DCFP_E_UNSUPPORTED;
    ResizeGeom G{};
    G.nlev = nlev;
    long long off = 0;
    G.cbeg[0] = 0;
    for (int l = 0; l < nlev; ++l) {
        const int Cl = level_chw[3 * l], sh = level_chw[3 * l + 1], sw = level_chw[3 * l + 2];
        if (Cl <= 0) return DCFP_E_BADDESC;
        if (sh < 1 || sh > kMaxS || sw < 1 || sw > kMaxS) return DCFP_E_UNSUPPORTED;
        G.sh[l] = sh; G.sw[l] = sw;
        G.cbeg[l + 1] = G.cbeg[l] + Cl;
        G.off[l] = off;
        off += (long long)N * Cl * sh * sw;
        G.scale_h[l] = host_scale(sh, H, align_corners);
        G.scale_w[l] = host_scale(sw, W, align_corners);
    }
    const int Ctot = G.cbeg[nlev];
    const int pitch = g_pitch ? g_pitch : W;
    if (pitch < W) return DCFP_E_BADDESC;
    if (g_nstride == 0) g_nstride = (int64_t)Ctot * H * pitch;
    if (g_nstride < (int64_t)Ctot * H * pitch) return DCFP_E_BADDESC;
    int R = kStageFloats / W;
    R = R < 1 ? 1 : (R > kMaxChunkRows ? kMaxChunkRows : R);
    const size_t lds = sizeof(float) * ((size_t)R * W + 3 * (size_t)W + kThreads);
    const bool v4 = W % 4 == 0 && pitch % 4 == 0 && g_nstride % 4 == 0 && dcfp_aligned16(g);
    const dim3 grid((unsigned)Ctot, (unsigned)N);
#define DCFP_PPM_RA(A, V)                                                                                       \
    hipLaunchKernelGGL((ppm_resize_adjoint_kernel<A, V>), grid, dim3(kThreads), lds, dcfp_s(stream), g,       \
                       (long long)g_nstride, pitch, H, W, dp, R, G)
    if (align_corners) {
        if (v4) DCFP_PPM_RA(true, 4); else DCFP_PPM_RA(true, 1);
    } else {
        if (v4) DCFP_PPM_RA(false, 4); else DCFP_PPM_RA(false, 1);
    }
#undef DCFP_PPM_RA
    DCFP_RETURN_LAUNCH();
}
