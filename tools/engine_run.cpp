// engine_run ENGINE.bin N H W input.raw [--u8] output.raw — runs a flat engine file (deploy.save_flat)
// once from C++: the HIP runtime and libdcfp_hip.so only, no Python.  input.raw is fp32 [N,3,H,W], or with --u8 uint8
// [N,H,W,3] (dense rows); output.raw receives the fp32 low-resolution logits [N,classes,h,w].  Exits non-zero with a
// message on any error.  Build: `make -C dcfp_amd/csrc engine_run`.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "dcfp_hip.h"

#define HIP_OK(call)                                                                             \
    do {                                                                                         \
        hipError_t e__ = (call);                                                                 \
        if (e__ != hipSuccess) {                                                                 \
            fprintf(stderr, "engine_run: %s: %s\n", #call, hipGetErrorString(e__));              \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

#define DCFP_CALL(call)                                                                          \
    do {                                                                                         \
        int s__ = (call);                                                                        \
        if (s__ != DCFP_OK) {                                                                    \
            fprintf(stderr, "engine_run: %s: status %d\n", #call, s__);                          \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

int main(int argc, char** argv) {
    std::vector<const char*> pos;
    bool u8 = false;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--u8")) u8 = true; else pos.push_back(argv[i]);
    }
    if (pos.size() != 6) {
        fprintf(stderr, "usage: %s ENGINE.bin N H W input.raw [--u8] output.raw\n", argv[0]);
        return 1;
    }
    const int N = atoi(pos[1]), H = atoi(pos[2]), W = atoi(pos[3]);
    char err[256];
    dcfp_engine_t eng = nullptr;
    if (dcfp_engine_open(pos[0], &eng, err, sizeof(err)) != DCFP_OK) {
        fprintf(stderr, "engine_run: %s\n", err);
        return 1;
    }
    dcfp_engine_info_t info;
    DCFP_CALL(dcfp_engine_info(eng, &info));
    int C = 0, h = 0, w = 0;
    DCFP_CALL(dcfp_engine_output_shape(eng, N, H, W, &C, &h, &w));
    const size_t ws_bytes = dcfp_engine_workspace_bytes(eng, N, H, W);
    if (ws_bytes == 0) {
        fprintf(stderr, "engine_run: a %dx%dx%d input is not supported\n", N, H, W);
        return 1;
    }
    const size_t in_bytes = (size_t)N * H * W * 3 * (u8 ? 1 : sizeof(float));
    const size_t out_bytes = (size_t)N * C * h * w * sizeof(float);
    std::vector<unsigned char> host_in(in_bytes);
    FILE* fp = fopen(pos[4], "rb");
    if (!fp || fread(host_in.data(), 1, in_bytes, fp) != in_bytes) {
        fprintf(stderr, "engine_run: %s does not hold %zu bytes\n", pos[4], in_bytes);
        return 1;
    }
    fclose(fp);

    void *weights = nullptr, *workspace = nullptr, *image = nullptr, *logits = nullptr;
    HIP_OK(hipMalloc(&weights, dcfp_engine_weight_bytes(eng)));
    HIP_OK(hipMalloc(&workspace, ws_bytes));
    HIP_OK(hipMalloc(&image, in_bytes));
    HIP_OK(hipMalloc(&logits, out_bytes));
    DCFP_CALL(dcfp_engine_upload(eng, weights, nullptr));
    HIP_OK(hipMemcpy(image, host_in.data(), in_bytes, hipMemcpyHostToDevice));
    if (u8)
        DCFP_CALL(dcfp_engine_run_u8(eng, weights, static_cast<const uint8_t*>(image), (size_t)3 * W, N, H, W, workspace,
                                     ws_bytes, static_cast<float*>(logits), nullptr));
    else
        DCFP_CALL(dcfp_engine_run_f32(eng, weights, static_cast<const float*>(image), N, H, W, workspace, ws_bytes,
                                      static_cast<float*>(logits), nullptr));
    HIP_OK(hipDeviceSynchronize());
    std::vector<unsigned char> host_out(out_bytes);
    HIP_OK(hipMemcpy(host_out.data(), logits, out_bytes, hipMemcpyDeviceToHost));
    fp = fopen(pos[5], "wb");
    if (!fp || fwrite(host_out.data(), 1, out_bytes, fp) != out_bytes || fclose(fp) != 0) {
        fprintf(stderr, "engine_run: cannot write %s\n", pos[5]);
        return 1;
    }
    HIP_OK(hipFree(logits));
    HIP_OK(hipFree(image));
    HIP_OK(hipFree(workspace));
    HIP_OK(hipFree(weights));
    dcfp_engine_close(eng);
    printf("engine_run: %s %dx%dx%d -> %dx%dx%dx%d logits (format %d)\n", u8 ? "uint8" : "fp32", N, H, W, N, C, h, w,
           info.format);
    return 0;
}
