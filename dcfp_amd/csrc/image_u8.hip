// image_u8.hip — the engine's uint8 input path: an interleaved 8-bit image (a camera frame, a decoded file) becomes
// the normalised NHWC fp16 buffer the first conv reads, through a 3 x 256 lookup table (deploy.input_table):
//     dst[n][y][x][c] = table[c * 256 + src[n][y][x][order[c]]]  (c < 3),  exact zeros for c = 3 .. C8-1.
// A pure lookup, so the result is defined exactly.  Bytes: 3 read + 2 * C8 written per pixel.
//
// One block converts kPix consecutive pixels of one row.  The 3 * kPix source bytes go to LDS in 16-byte loads
// wherever the address is 16-byte aligned inside the row (row pitch and base are arbitrary), the bytes before the
// first and after the last such vector one by one; the table sits in LDS next to them.  Then lane i takes pixel
// i, i + 256, ...: consecutive lanes store consecutive 16-byte chunks of the destination.
#include "common.h"

namespace {

typedef _Float16 h8_t __attribute__((ext_vector_type(8)));

constexpr int kPix = 1024;              // pixels per block
constexpr int kBytes = 3 * kPix;        // their source bytes

__global__ __launch_bounds__(256) void image_u8_kernel(const unsigned char* __restrict__ src, long row_pitch, int H,
                                                       int W, const _Float16* __restrict__ table, int o0, int o1,
                                                       int o2, h8_t* __restrict__ dst, int c8n, int chunks) {
    __shared__ __attribute__((aligned(16))) unsigned char raw[kBytes + 32];
    __shared__ __attribute__((aligned(16))) _Float16 lut[3 * 256];
    const int tid = threadIdx.x;
    const int chunk = blockIdx.x % chunks;
    const long row = blockIdx.x / chunks;                    // n * H + y
    const int x0 = chunk * kPix;
    const int npix = min(kPix, W - x0);
    const unsigned char* base = src + row * row_pitch + 3l * x0;   // first byte of the block's pixels
    const int nbytes = 3 * npix;
    // LDS byte j + head holds base[j]: LDS keeps the source's alignment modulo 16
    const int head = (int)(reinterpret_cast<uintptr_t>(base) & 15u);
    const int lead = min(nbytes, (16 - head) & 15);          // bytes before the first aligned vector
    const int nvec = (nbytes - lead) / 16;
    const int tail0 = lead + nvec * 16;                      // first byte after the last whole vector
    for (int v = tid; v < nvec; v += 256)
        *reinterpret_cast<uint4*>(&raw[head + lead + 16 * v]) = *reinterpret_cast<const uint4*>(base + lead + 16 * v);
    if (tid < lead) raw[head + tid] = base[tid];
    if (tid >= 64 && tid - 64 < nbytes - tail0) raw[head + tail0 + tid - 64] = base[tail0 + tid - 64];
    for (int i = tid; i < 3 * 256 / 8; i += 256)
        reinterpret_cast<h8_t*>(lut)[i] = reinterpret_cast<const h8_t*>(table)[i];
    __syncthreads();
    h8_t* out = dst + (row * W + x0) * c8n;
    const int total = npix * c8n;
    for (int i = tid; i < total; i += 256) {
        const int p = i / c8n, ch = i - p * c8n;
        h8_t o = {0, 0, 0, 0, 0, 0, 0, 0};
        if (ch == 0) {
            const unsigned char* px = &raw[head + 3 * p];
            o[0] = lut[px[o0]];
            o[1] = lut[256 + px[o1]];
            o[2] = lut[512 + px[o2]];
        }
        out[i] = o;
    }
}

}  // namespace

extern "C" {

int dcfp_image_u8_hwc_to_nhwc_f16(const uint8_t* src, size_t row_pitch_bytes, int N, int H, int W, const void* table,
                                  const int* order, void* dst, int C8, dcfp_stream_t stream) {
    if (!src || !table || !order || !dst || N <= 0 || H <= 0 || W <= 0 || C8 < 8 || (C8 & 7)) return DCFP_E_BADDESC;
    if (row_pitch_bytes < 3 * (size_t)W || !dcfp_aligned16(table) || !dcfp_aligned16(dst)) return DCFP_E_BADDESC;
    for (int c = 0; c < 3; ++c)
        if (order[c] < 0 || order[c] > 2) return DCFP_E_BADDESC;
    const int chunks = (W + kPix - 1) / kPix;
    const long blocks = (long)N * H * chunks;
    if (blocks >= (1l << 31) || (long)N * H * W >= (1l << 31) || row_pitch_bytes > (size_t)1 << 40) return DCFP_E_UNSUPPORTED;
    hipLaunchKernelGGL(image_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, dcfp_s(stream), src, (long)row_pitch_bytes,
                       H, W, reinterpret_cast<const _Float16*>(table), order[0], order[1], order[2],
                       reinterpret_cast<h8_t*>(dst), C8 / 8, chunks);
    DCFP_RETURN_LAUNCH();
}

}  // extern "C"
