// png.hip — label maps to finished zlib streams of 8-bit PNGs, on the device.
//
// For every (image n, lookup table p) the bytes b[y][x] = lut[p][pred[n][y][x] & 255] are never stored: a row's
// filtered bytes f = {2, (b[y][x] - b[y-1][x]) mod 256} (PNG filter type Up) are formed in LDS from the int32 row and
// the row above it, and turned into one fixed-Huffman deflate block followed by an empty stored block, which ends the
// row's piece on a byte boundary.  The token rule is closed form per maximal run of equal filtered bytes (value v,
// length L): the literal v, (L-1)/258 matches of length 258 at distance 1, then with r = (L-1)%258 one match of
// length r if r >= 3, else r literals.  Three launches, integer arithmetic only:
//   row kernel    : one workgroup per (n, p, y); lane t owns ceil((W+1)/NT) consecutive filtered bytes.  Run starts
//                   come from a neighbour compare, the start of the next run from an exclusive suffix minimum over the
//                   lanes, the bit offset of a lane's runs from an exclusive prefix sum of their closed-form bit
//                   counts; the lane that owns a run start ORs the run's tokens into an LDS bit buffer (32-bit LDS
//                   atomics).  The piece goes to a scratch slot of fixed pitch, its length and the row's Adler-32
//                   partials (sum f, sum (len-i) f[i], both mod 65521) to arrays.
//   stream kernel : one workgroup per (n, p): exclusive scan of the H piece lengths, Adler-32 of the stream from the
//                   row partials in row order (a prefix sum again), the stream's length.
//   pack kernel   : one wave per row copies the piece to its place in the compacted output; the first and last row of
//                   a stream add the header 78 01 and the trailer 03 00 + Adler-32.
// Every output byte is stored once by a fixed lane and OR is commutative, so two calls give the same bytes.
#include "common.h"

namespace {

constexpr int kMaxH = 4096, kMaxW = 8192, kMaxP = 4;
constexpr unsigned kAdler = 65521u;
constexpr int kNoStart = 0x7fffffff;

__host__ __device__ inline long long row_bound(int W) { return (9LL * (W + 1) + 13 + 7) / 8 + 4; }
__host__ __device__ inline long long row_pitch(int W) { return (row_bound(W) + 3) & ~3LL; }

__device__ __forceinline__ int lit_bits(unsigned v) { return v < 144u ? 8 : 9; }

// RFC 1951 length code of a match of length r (3 .. 257) and its number of extra bits
__device__ __forceinline__ void len_code(int r, int& code, int& extra) {
    const int x = r - 3;
    extra = x < 8 ? 0 : 29 - __clz(x);
    code = x < 8 ? 257 + x : 261 + 4 * extra + ((x - (4 << extra)) >> extra);
}

__device__ __forceinline__ int run_bits(unsigned v, int L) {
    const int nm = (L - 1) / 258, r = (L - 1) % 258, lb = lit_bits(v);
    int b = lb + 13 * nm;
    if (r >= 3) {
        int code, extra;
        len_code(r, code, extra);
        b += (code < 280 ? 7 : 8) + extra + 5;
    } else {
        b += r * lb;
    }
    return b;
}

// nb <= 32 bits of val, least significant first, at bit `pos` of the row's bit buffer
__device__ __forceinline__ void put_bits(unsigned* buf, int pos, unsigned val, int nb) {
    const int w = pos >> 5, sh = pos & 31;
    atomicOr(&buf[w], val << sh);
    if (sh + nb > 32) atomicOr(&buf[w + 1], val >> (32 - sh));
}

__device__ __forceinline__ void put_run(unsigned* buf, int pos, unsigned v, int L) {
    const int nm = (L - 1) / 258, r = (L - 1) % 258, lb = lit_bits(v);
    const unsigned lit = __brev(v < 144u ? 0x30u + v : 0x190u + (v - 144u)) >> (32 - lb);   // Huffman codes go MSB first
    put_bits(buf, pos, lit, lb);
    pos += lb;
    for (int m = 0; m < nm; ++m) {                   // length 258 = code 285 (8 bits 11000101), distance code 0 (5 bits)
        put_bits(buf, pos, 0xA3u, 13);
        pos += 13;
    }
    if (r >= 3) {
        int code, extra;
        len_code(r, code, extra);
        const int cb = code < 280 ? 7 : 8;
        const unsigned hc = code < 280 ? (unsigned)(code - 256) : 0xC0u + (unsigned)(code - 280);
        const unsigned ex = (unsigned)(r - 3) & ((1u << extra) - 1u);
        put_bits(buf, pos, (__brev(hc) >> (32 - cb)) | (ex << cb), cb + extra + 5);
    } else {
        for (int m = 0; m < r; ++m) {
            put_bits(buf, pos, lit, lb);
            pos += lb;
        }
    }
}

__device__ __forceinline__ int wave_suffix_min_i(int v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_down(v, off, 64);
        if (lane + off < 64) v = min(v, t);
    }
    return v;
}
__device__ __forceinline__ unsigned wave_prefix_sum_u(unsigned v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}

// exclusive prefix sum over the NT threads of a block, and the block's total; sm: NT/64 words, free on return
template <int NT>
__device__ __forceinline__ unsigned block_excl_sum(unsigned v, unsigned* sm, unsigned& total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const unsigned incl = wave_prefix_sum_u(v, lane);
    if (lane == 63) sm[wid] = incl;
    __syncthreads();
    unsigned before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        const unsigned t = sm[w];
        if (w < wid) before += t;
        total += t;
    }
    __syncthreads();
    return before + incl - v;
}

template <int NT>
__global__ __launch_bounds__(NT) void png_row_kernel(const int32_t* __restrict__ pred, const uint8_t* __restrict__ luts,
                                                     uint8_t* __restrict__ scratch, uint32_t* __restrict__ rowlen,
                                                     uint32_t* __restrict__ rowA, uint32_t* __restrict__ rowB, int H,
                                                     int W, int P) {
    extern __shared__ unsigned dyn[];                // bit buffer: pitch bytes; filtered row: W + 1 bytes
    __shared__ uint8_t lut[256];
    __shared__ unsigned sm[NT / 64];
    __shared__ int smi[NT / 64];
    const long long pitch = row_pitch(W);
    unsigned* bits = dyn;
    uint8_t* f = reinterpret_cast<uint8_t*>(dyn) + pitch;
    const long long r = blockIdx.x;                  // (n*P + p)*H + y
    const int y = (int)(r % H);
    const long long s = r / H;
    const int p = (int)(s % P);
    const long long n = s / P;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int len = W + 1;

    for (int t = tid; t < 256; t += NT) lut[t] = luts[p * 256 + t];
    for (int w = tid; w < (int)(pitch >> 2); w += NT) bits[w] = 0u;
    __syncthreads();
    const int32_t* row = pred + (n * H + y) * (long long)W;
    if (tid == 0) f[0] = 2;
    for (int x = tid; x < W; x += NT) {
        const unsigned cur = lut[row[x] & 255];
        const unsigned up = y > 0 ? lut[row[x - W] & 255] : 0u;     // the row above: a recent row, from L2
        f[1 + x] = (uint8_t)(cur - up);
    }
    __syncthreads();

    const int K = (len + NT - 1) / NT;
    const int i0 = min(len, tid * K), i1 = min(len, i0 + K);
    // the lane's first run start, and its Adler partials
    int first = kNoStart;
    unsigned sa = 0, sb = 0;                         // <= 33 * 255 * 8193: no overflow
    {
        unsigned prev = i0 > 0 && i0 < len ? f[i0 - 1] : 0x100u;
        for (int i = i0; i < i1; ++i) {
            const unsigned v = f[i];
            if (v != prev && first == kNoStart) first = i;
            prev = v;
            sa += v;
            sb += (unsigned)(len - i) * v;
        }
    }
    // start of the first run after this lane's bytes
    int next0;
    {
        const int incl = wave_suffix_min_i(first, lane);
        int excl = __shfl_down(incl, 1, 64);
        if (lane == 63) excl = kNoStart;
        if (lane == 0) smi[wid] = incl;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < NT / 64; ++w)
            if (w > wid) excl = min(excl, smi[w]);
        next0 = min(excl, len);
    }
    // bit count of the runs that start in this lane's bytes
    unsigned mybits = 0;
    {
        int next = next0;
        for (int i = i1 - 1; i >= i0; --i) {
            const unsigned v = f[i];
            if (i == 0 || f[i - 1] != v) {
                mybits += (unsigned)run_bits(v, next - i);
                next = i;
            }
        }
    }
    unsigned total;
    const unsigned before = block_excl_sum<NT>(mybits, sm, total);
    {
        int next = next0, pos = 3 + (int)(before + mybits);
        for (int i = i1 - 1; i >= i0; --i) {
            const unsigned v = f[i];
            if (i == 0 || f[i - 1] != v) {
                pos -= run_bits(v, next - i);
                put_run(bits, pos, v, next - i);
                next = i;
            }
        }
    }
    if (tid == 0) atomicOr(&bits[0], 2u);            // BFINAL = 0, BTYPE = 01
    // end-of-block (7 zero bits), the stored block's header (3 zero bits) and its padding are the zeros already there
    const unsigned body = (total + 13u + 7u) >> 3;
    __syncthreads();
    if (tid == 0) {                                  // LEN = 0, NLEN = ffff
        uint8_t* bytes = reinterpret_cast<uint8_t*>(bits);
        bytes[body + 2] = 0xff;
        bytes[body + 3] = 0xff;
    }
    // Adler partials of the row
    sa %= kAdler;
    sb %= kAdler;
    unsigned ta, tb;
    block_excl_sum<NT>(sa, sm, ta);                  // (its barriers also publish the two bytes above)
    block_excl_sum<NT>(sb, sm, tb);
    if (tid == 0) {
        rowlen[r] = body + 4u;
        rowA[r] = ta % kAdler;
        rowB[r] = tb % kAdler;
    }
    unsigned* dst = reinterpret_cast<unsigned*>(scratch + r * pitch);
    for (int w = tid; w < (int)((body + 4u + 3u) >> 2); w += NT) dst[w] = bits[w];
}

// one workgroup per stream: row offsets inside the stream, the stream's length and Adler-32
__global__ __launch_bounds__(256) void png_stream_kernel(const uint32_t* __restrict__ rowlen,
                                                         const uint32_t* __restrict__ rowA,
                                                         const uint32_t* __restrict__ rowB, uint32_t* __restrict__ rowoff,
                                                         uint32_t* __restrict__ adler, int64_t* __restrict__ lengths,
                                                         int H, int W) {
    __shared__ unsigned sm[4];
    const long long s = blockIdx.x;
    const int tid = threadIdx.x;
    const unsigned len = (unsigned)W + 1u;
    unsigned off = 2u, a = 1u;                       // after the header 78 01; Adler-32 starts at a = 1, b = 0
    unsigned long long b = 0;                        // this thread's share of b, reduced at the end
    for (int y0 = 0; y0 < H; y0 += 256) {
        const int y = y0 + tid;
        const bool in = y < H;
        const unsigned l = in ? rowlen[s * H + y] : 0u, ra = in ? rowA[s * H + y] : 0u;
        unsigned tl, tA;
        const unsigned el = block_excl_sum<256>(l, sm, tl);
        const unsigned ea = block_excl_sum<256>(ra, sm, tA);     // <= 4096 * 65520 over a stream: no overflow
        if (in) {
            rowoff[s * H + y] = off + el;
            // a row of `len` bytes met with (a0, b): b += len * a0 + sum (len - i) f[i]
            b += (unsigned long long)len * ((a + ea) % kAdler) + rowB[s * H + y];
        }
        off += tl;
        a += tA;
    }
    unsigned tb;
    block_excl_sum<256>((unsigned)(b % kAdler), sm, tb);
    if (tid == 0) {
        adler[s] = ((tb % kAdler) << 16) | (a % kAdler);
        lengths[s] = (int64_t)off + 6;               // 03 00 and the four Adler bytes
    }
}

// one wave per row: the piece to its place in the compacted output
__global__ __launch_bounds__(256) void png_pack_kernel(const uint8_t* __restrict__ scratch,
                                                       const uint32_t* __restrict__ rowlen,
                                                       const uint32_t* __restrict__ rowoff,
                                                       const uint32_t* __restrict__ adler,
                                                       const int64_t* __restrict__ lengths, uint8_t* __restrict__ out,
                                                       int64_t* __restrict__ offsets, long long rows, int H,
                                                       long long pitch) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                           // (no barrier below)
    const long long s = r / H;
    const int y = (int)(r % H);
    long long base = 0;                              // streams lie one after the other
    for (long long q = lane; q < s; q += 64) base += lengths[q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) base += __shfl_xor(base, off, 64);
    uint8_t* dst = out + base;
    const uint8_t* src = scratch + r * pitch;
    const unsigned n = rowlen[r], o = rowoff[r];
    for (unsigned i = lane; i < n; i += 64) dst[o + i] = src[i];
    if (y == 0 && lane == 0) {
        dst[0] = 0x78;
        dst[1] = 0x01;
        offsets[s] = base;
    }
    if (y == H - 1 && lane < 6) {
        const unsigned ad = adler[s];
        const unsigned v = lane == 0 ? 0x03u : lane == 1 ? 0u : (ad >> (8 * (5 - lane))) & 0xffu;   // big endian
        dst[o + n + lane] = (uint8_t)v;
    }
}

// scratch slots, then rowlen, rowA, rowB, rowoff (uint32 per row), then adler (uint32 per stream)
size_t ws_bytes_of(long long rows, long long streams, int W) {
    return (size_t)rows * (size_t)row_pitch(W) + (size_t)rows * 16 + (size_t)streams * 4;
}

}  // namespace

extern "C" size_t dcfp_png_deflate_bound(int H, int W) {
    if (H <= 0 || W <= 0 || H > kMaxH || W > kMaxW) return 0;
    return (size_t)2 + (size_t)H * (size_t)row_bound(W) + 2 + 4;
}

extern "C" size_t dcfp_png_deflate_workspace_bytes(int N, int H, int W, int P) {
    if (N <= 0 || P < 1 || P > kMaxP || H <= 0 || W <= 0 || H > kMaxH || W > kMaxW) return 0;
    const long long streams = (long long)N * P, rows = streams * H;
    if (rows > 0x7fffffffLL) return 0;
    return ws_bytes_of(rows, streams, W);
}

extern "C" int dcfp_png_deflate_labels_i32(const int32_t* pred, int N, int H, int W, const uint8_t* luts, int P,
                                           uint8_t* out, size_t out_bytes, int64_t* offsets, int64_t* lengths,
                                           void* ws, size_t ws_bytes, dcfp_stream_t stream) {
    if (!pred || !luts || !out || !offsets || !lengths || !ws || N <= 0 || H <= 0 || W <= 0 || P < 1 || P > kMaxP ||
        (reinterpret_cast<uintptr_t>(ws) & 3u))
        return DCFP_E_BADDESC;
    if (H > kMaxH || W > kMaxW) return DCFP_E_UNSUPPORTED;
    const long long streams = (long long)N * P, rows = streams * H;
    if (rows > 0x7fffffffLL) return DCFP_E_UNSUPPORTED;
    if (out_bytes < (size_t)streams * dcfp_png_deflate_bound(H, W)) return DCFP_E_BADDESC;
    if (ws_bytes < ws_bytes_of(rows, streams, W)) return DCFP_E_WORKSPACE;
    const long long pitch = row_pitch(W);
    uint8_t* scratch = static_cast<uint8_t*>(ws);
    uint32_t* rowlen = reinterpret_cast<uint32_t*>(scratch + rows * pitch);
    uint32_t *rowA = rowlen + rows, *rowB = rowA + rows, *rowoff = rowB + rows, *adler = rowoff + rows;
    const size_t lds = (size_t)pitch + (size_t)((W + 1 + 3) & ~3);
    if (W + 1 <= 512)                                // narrow rows: one wave, at most 8 bytes per lane
        hipLaunchKernelGGL(png_row_kernel<64>, dim3((unsigned)rows), dim3(64), lds, dcfp_s(stream), pred, luts, scratch,
                           rowlen, rowA, rowB, H, W, P);
    else
        hipLaunchKernelGGL(png_row_kernel<256>, dim3((unsigned)rows), dim3(256), lds, dcfp_s(stream), pred, luts,
                           scratch, rowlen, rowA, rowB, H, W, P);
    hipLaunchKernelGGL(png_stream_kernel, dim3((unsigned)streams), dim3(256), 0, dcfp_s(stream), rowlen, rowA, rowB,
                       rowoff, adler, lengths, H, W);
    hipLaunchKernelGGL(png_pack_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, dcfp_s(stream), scratch, rowlen,
                       rowoff, adler, lengths, out, offsets, rows, H, pitch);
    DCFP_RETURN_LAUNCH();
}
