// engine_rt.hip — the C engine runtime: loads a flat engine file and runs its plan through the
// library's own extern "C" entry points, in plan order, on the caller's stream.  No kernel and no dispatch lives here.
// The caller owns every device buffer; a handle owns host memory only: the parsed file and, per input shape, the
// cached shape program (buffer sizes, slot offsets, workspace size).  It is a port of Engine.buffer_shapes, the
// liveness slot assignment of Engine.__init__ and the workspace sizing of Engine._program (dcfp_amd/deploy.py).
#include <stdio.h>

#include <algorithm>
#include <new>

#include "common.h"
#include "engine_file.h"

using namespace dcfp_efile;

namespace {

constexpr size_t kSlotAlign = 256;
constexpr int kMaxSide = 32768;      // what the conv and resize kernels take
constexpr int kMaxPrograms = 8;      // cached shape programs per handle

size_t r256(size_t v) { return (v + kSlotAlign - 1) / kSlotAlign * kSlotAlign; }
int r8(int c) { return (c + 7) / 8 * 8; }
int esize(int fmt) { return fmt == FMT_F8 ? 1 : 2; }

struct Program {
    int N = 0, H = 0, W = 0;
    int status = DCFP_OK;               // DCFP_E_BADDESC: input too small; DCFP_E_UNSUPPORTED: a size no kernel takes
    std::vector<int> h, w;              // per buffer; 0: never written
    int out_h = 0, out_w = 0;           // the classifier's map
    std::vector<size_t> slot_off;       // per slot, into the caller's workspace
    std::vector<size_t> ws_of;          // per record: bytes of pool workspace it needs
    size_t ws_off = 0, ws_bytes = 0, total = 0;
};

}  // namespace

struct dcfp_engine {
    File file;
    std::vector<int> slot_of;           // buffer -> slot (-1: no record names the buffer)
    int n_slots = 0;
    std::vector<Program> programs;      // most recently built last
};

namespace {

// Engine.__init__: a buffer lives from the first to the last record naming it; buffers with disjoint lifetimes share
// a slot (a freed slot is reused last-in first-out), the same for every input shape.
void assign_slots(dcfp_engine& E) {
    const File& f = E.file;
    const int nb = (int)f.buffers.size(), nr = (int)f.records.size();
    std::vector<int> first(nb, -2), last(nb, -2);
    first[0] = -1;
    for (int i = 0; i < nr; ++i) {
        const Record& r = f.records[i];
        int ids[7] = {r.src, r.dst, r.res, -1, -1, -1, -1};
        if (r.op == OP_PYRAMID)
            for (int l = 0; l < r.nlev; ++l) ids[3 + l] = r.dsts[l];
        for (int b : ids)
            if (b >= 0) {
                if (first[b] == -2) first[b] = i;
                last[b] = i;
            }
    }
    E.slot_of.assign(nb, -1);
    std::vector<int> free_slots;
    for (int i = -1; i < nr; ++i) {
        for (int b = 0; b < nb; ++b)            // (ascending buffer id, as the Python engine sorts them)
            if (first[b] == i) {
                if (!free_slots.empty()) {
                    E.slot_of[b] = free_slots.back();
                    free_slots.pop_back();
                } else {
                    E.slot_of[b] = E.n_slots++;
                }
            }
        for (int b = 0; b < nb; ++b)
            if (last[b] == i) free_slots.push_back(E.slot_of[b]);
    }
}

bool set_shape(Program& P, int b, int h, int w) {   // hw.setdefault(b, o) == o
    if (P.h[b] == 0) { P.h[b] = h; P.w[b] = w; }
    return P.h[b] == h && P.w[b] == w;
}

// Engine.buffer_shapes + the sizing half of Engine._program for one (N, H, W)
void build_program(const dcfp_engine& E, int N, int H, int W, Program& P) {
    const File& f = E.file;
    const int nb = (int)f.buffers.size(), nr = (int)f.records.size();
    P = Program{};
    P.N = N; P.H = H; P.W = W;
    if (N < 1 || H < 1 || W < 1) { P.status = DCFP_E_BADDESC; return; }
    if (N > 65535 || H > kMaxSide || W > kMaxSide || (int64_t)N * H * W >= (1ll << 31)) { P.status = DCFP_E_UNSUPPORTED; return; }
    P.h.assign(nb, 0); P.w.assign(nb, 0);
    P.ws_of.assign(nr, 0);
    P.h[0] = H; P.w[0] = W;
    for (int i = 0; i < nr; ++i) {
        const Record& r = f.records[i];
        const int h = P.h[r.src], w = P.w[r.src];   // (the parser made sure an earlier record wrote it)
        int oh = 0, ow = 0;
        switch (r.op) {
        case OP_CONV: {
            const int ext = r.dil * (r.k - 1) + 1;
            if (h + 2 * r.pad < ext || w + 2 * r.pad < ext) { P.status = DCFP_E_BADDESC; return; }
            oh = (h + 2 * r.pad - ext) / r.stride + 1;
            ow = (w + 2 * r.pad - ext) / r.stride + 1;
            break;
        }
        case OP_MAXPOOL: oh = (h - 1) / 2 + 1; ow = (w - 1) / 2 + 1; break;
        case OP_AVGPOOL: oh = ow = 1; break;
        case OP_CAST: oh = h; ow = w; break;
        case OP_BROADCAST:
        case OP_RESIZE: oh = P.h[r.dst]; ow = P.w[r.dst]; break;
        case OP_PYRAMID:
            for (int l = 0; l < r.nlev; ++l)
                if (!set_shape(P, r.dsts[l], r.sizes[l], r.sizes[l])) { P.status = DCFP_E_BADDESC; return; }
            oh = ow = r.sizes[0];
            break;
        }
        if (oh < 1 || ow < 1) { P.status = DCFP_E_BADDESC; return; }
        if (oh > kMaxSide || ow > kMaxSide || (int64_t)N * oh * ow >= (1ll << 31)) { P.status = DCFP_E_UNSUPPORTED; return; }
        if (r.op == OP_CONV && r.f32) {
            P.out_h = oh; P.out_w = ow;
        } else if (!set_shape(P, r.dst, oh, ow)) {
            P.status = DCFP_E_BADDESC; return;
        }
        if (r.res >= 0 && (P.h[r.res] != oh || P.w[r.res] != ow)) { P.status = DCFP_E_BADDESC; return; }
        if (r.op == OP_AVGPOOL) {
            P.ws_of[i] = dcfp_avgpool_nhwc_f16_workspace_bytes(N, f.buffers[r.src].pitch, (int64_t)h * w);
        } else if (r.op == OP_PYRAMID) {
            P.ws_of[i] = dcfp_pyramid_pool_nhwc_f16_workspace_bytes(N, h, w, r.c8, r.nlev, r.sizes);
            if (P.ws_of[i] == 0) { P.status = DCFP_E_UNSUPPORTED; return; }
        }
        P.ws_bytes = std::max(P.ws_bytes, P.ws_of[i]);
    }
    std::vector<size_t> need(E.n_slots, 0);
    for (int b = 0; b < nb; ++b)
        if (P.h[b] > 0 && E.slot_of[b] >= 0)
            need[E.slot_of[b]] = std::max(need[E.slot_of[b]], (size_t)N * P.h[b] * P.w[b] * f.buffers[b].pitch *
                                                                   esize(f.buffers[b].fmt));
    P.slot_off.assign(E.n_slots, 0);
    size_t at = 0;
    for (int s = 0; s < E.n_slots; ++s) {
        P.slot_off[s] = at;
        at += r256(need[s]);
    }
    P.ws_off = at;                      // the pool partial sums follow the slots
    P.total = at + P.ws_bytes;
}

// (never null; on an allocation failure a program that says "unsupported" - nothing throws across the ABI)
const Program* program_or_throw(dcfp_engine* E, int N, int H, int W);
const Program* program(dcfp_engine* E, int N, int H, int W) {
    static const Program kNoMemory = [] { Program p; p.status = DCFP_E_UNSUPPORTED; return p; }();
    try {
        return program_or_throw(E, N, H, W);
    } catch (...) {
        E->programs.clear();
        return &kNoMemory;
    }
}

const Program* program_or_throw(dcfp_engine* E, int N, int H, int W) {
    for (size_t i = 0; i < E->programs.size(); ++i)
        if (E->programs[i].N == N && E->programs[i].H == H && E->programs[i].W == W) {
            std::rotate(E->programs.begin() + i, E->programs.begin() + i + 1, E->programs.end());
            return &E->programs.back();
        }
    if ((int)E->programs.size() >= kMaxPrograms) E->programs.erase(E->programs.begin());
    E->programs.emplace_back();
    build_program(*E, N, H, W, E->programs.back());
    return &E->programs.back();
}

int open_parsed(File&& f, dcfp_engine_t* out) {
    dcfp_engine* E = new (std::nothrow) dcfp_engine();
    if (!E) return DCFP_E_BADDESC;
    E->file = std::move(f);
    try {
        assign_slots(*E);
    } catch (...) {
        delete E;
        return DCFP_E_BADDESC;
    }
    *out = E;
    return DCFP_OK;
}

void no_memory(char* err, size_t errlen) {
    if (err && errlen) snprintf(err, errlen, "engine file: out of memory");
}

size_t table_offset(const dcfp_engine* E) { return r256(E->file.weights_size); }

// the plan, record by record, through the library's entry points (the order and the arguments of Engine._program)
int run_plan(dcfp_engine* E, const Program& P, const void* dev_weights, void* workspace, float* logits, hipStream_t hs) {
    const File& f = E->file;
    dcfp_stream_t s = reinterpret_cast<dcfp_stream_t>(hs);
    char* base = static_cast<char*>(workspace);
    const char* wts = static_cast<const char*>(dev_weights);
    auto ptr = [&](int b) -> void* { return base + P.slot_off[E->slot_of[b]]; };
    auto tensor = [&](int t) -> const void* { return wts + f.tensors[t].offset; };
    void* pool_ws = base + P.ws_off;
    const int N = P.N;
    for (size_t i = 0; i < f.records.size(); ++i) {
        const Record& r = f.records[i];
        const int h = P.h[r.src], w = P.w[r.src];
        const bool f8 = r.fmt == FMT_F8, f32 = r.op == OP_CONV && r.f32;
        const int ho = f32 ? P.out_h : P.h[r.dst], wo = f32 ? P.out_w : P.w[r.dst];
        const int sp = f.buffers[r.src].pitch, dp = f32 ? 0 : f.buffers[r.dst].pitch;
        const int rp = r.res >= 0 ? f.buffers[r.res].pitch : 0;
        int st = DCFP_OK;
        switch (r.op) {
        case OP_CONV:
            if (f8) {
                const DcfpConvF8Desc d = {N, h, w, r.cin8, sp, r.cout, r.k, r.stride, r.pad, r.dil, ho, wo, dp, r.y_off,
                                          rp, 0, r.relu, r.res_mul};
                const float* mul = static_cast<const float*>(tensor(r.t_a));
                const float* add = static_cast<const float*>(tensor(r.t_b));
                st = f32 ? dcfp_conv2d_fwd_f8_nhwc_to_f32_nchw(&d, ptr(r.src), tensor(r.t_w), mul, add, logits, s)
                         : dcfp_conv2d_fwd_f8_nhwc(&d, ptr(r.src), tensor(r.t_w), mul, add,
                                                   r.res >= 0 ? ptr(r.res) : nullptr, ptr(r.dst), s);
            } else {
                const DcfpConvF16Desc d = {N, h, w, r.cin8, sp, f32 ? r.cout : r8(r.cout), r.k, r.stride, r.pad, r.dil,
                                           ho, wo, dp, r.y_off, rp, 0, r.relu};
                const float* shift = static_cast<const float*>(tensor(r.t_a));
                st = f32 ? dcfp_conv2d_fwd_f16_nhwc_to_f32_nchw(&d, ptr(r.src), tensor(r.t_w), shift, logits, s)
                         : dcfp_conv2d_fwd_f16_nhwc(&d, ptr(r.src), tensor(r.t_w), shift,
                                                    r.res >= 0 ? ptr(r.res) : nullptr, ptr(r.dst), s);
            }
            break;
        case OP_MAXPOOL:
            st = f8 ? dcfp_maxpool3x3s2_nhwc_f8(ptr(r.src), ptr(r.dst), N, h, w, sp, sp, ho, wo, dp, s)
                    : dcfp_maxpool3x3s2_nhwc_f16(ptr(r.src), ptr(r.dst), N, h, w, sp, sp, ho, wo, dp, s);
            break;
        case OP_AVGPOOL:
            st = f8 ? dcfp_avgpool_nhwc_f8_to_f16(ptr(r.src), ptr(r.dst), N, (int64_t)h * w, sp, sp, dp, r.scale, pool_ws,
                                                  P.ws_of[i], s)
                    : dcfp_avgpool_nhwc_f16(ptr(r.src), ptr(r.dst), N, (int64_t)h * w, sp, sp, dp, pool_ws, P.ws_of[i], s);
            break;
        case OP_BROADCAST:
            st = f8 ? dcfp_broadcast_nhwc_f16_to_f8(ptr(r.src), sp, ptr(r.dst), N, (int64_t)ho * wo, r.c, dp, r.y_off,
                                                    r.scale, s)
                    : dcfp_broadcast_nhwc_f16(ptr(r.src), sp, ptr(r.dst), N, (int64_t)ho * wo, sp, dp, r.y_off, s);
            break;
        case OP_CAST:
            st = dcfp_cast_nhwc_f16_to_f8(ptr(r.src), sp, ptr(r.dst), dp, r.y_off, (int64_t)N * h * w, r.c, r.scale, s);
            break;
        case OP_RESIZE:
            st = dcfp_resize_bilinear_nhwc_f16(ptr(r.src), N, h, w, sp, sp, ptr(r.dst), ho, wo, dp, r.y_off, r.align, s);
            break;
        case OP_PYRAMID: {
            void* outs[kPyramidMaxLevels] = {};
            int pitches[kPyramidMaxLevels] = {};
            for (int l = 0; l < r.nlev; ++l) {
                outs[l] = ptr(r.dsts[l]);
                pitches[l] = f.buffers[r.dsts[l]].pitch;
            }
            st = dcfp_pyramid_pool_nhwc_f16(ptr(r.src), N, h, w, r.c8, sp, r.x_off, r.nlev, r.sizes, outs, pitches,
                                            pool_ws, P.ws_of[i], s);
            break;
        }
        }
        if (st != DCFP_OK) return st;   // a launch failure: the kernel's status, and nothing further is launched
    }
    return DCFP_OK;
}

// everything that can be refused is refused here, before the first launch
int check_run(dcfp_engine* E, const void* dev_weights, const void* image, int N, int H, int W, void* workspace,
              size_t workspace_bytes, float* logits, const Program** P) {
    if (!E || !dev_weights || !image || !logits || !dcfp_aligned16(dev_weights)) return DCFP_E_BADDESC;
    *P = program(E, N, H, W);
    if ((*P)->status != DCFP_OK) return (*P)->status;
    if (!workspace || workspace_bytes < (*P)->total) return DCFP_E_WORKSPACE;
    if (!dcfp_aligned16(workspace)) return DCFP_E_BADDESC;
    return DCFP_OK;
}

}  // namespace

extern "C" {

int dcfp_engine_open(const char* path, dcfp_engine_t* out, char* err, size_t errlen) {
    if (err && errlen) err[0] = 0;
    if (!out) return DCFP_E_BADDESC;
    *out = nullptr;
    try {
        File f;
        if (!load(path, f, err, errlen)) return DCFP_E_BADDESC;
        return open_parsed(std::move(f), out);
    } catch (...) {
        no_memory(err, errlen);
        return DCFP_E_BADDESC;
    }
}

int dcfp_engine_open_memory(const void* bytes, size_t n, dcfp_engine_t* out, char* err, size_t errlen) {
    if (err && errlen) err[0] = 0;
    if (!out) return DCFP_E_BADDESC;
    *out = nullptr;
    try {
        File f;
        if (!parse(bytes, n, f, err, errlen)) return DCFP_E_BADDESC;
        return open_parsed(std::move(f), out);
    } catch (...) {
        no_memory(err, errlen);
        return DCFP_E_BADDESC;
    }
}

void dcfp_engine_close(dcfp_engine_t e) { delete e; }

int dcfp_engine_info(dcfp_engine_t e, dcfp_engine_info_t* out) {
    if (!e || !out) return DCFP_E_BADDESC;
    const Meta& m = e->file.meta;
    out->format = m.format;
    out->num_classes = m.num_classes;
    out->in_channels = m.in_channels;
    out->align_corner = m.align_corner;
    out->model = m.model;
    out->n_records = m.n_records;
    out->n_buffers = m.n_buffers;
    out->n_slots = e->n_slots;
    out->has_input_table = e->file.has_input ? 1 : 0;
    return DCFP_OK;
}

size_t dcfp_engine_weight_bytes(dcfp_engine_t e) {
    if (!e) return 0;
    return table_offset(e) + (e->file.has_input ? kTableBytes : 0);
}

int dcfp_engine_upload(dcfp_engine_t e, void* dev_weights, dcfp_stream_t stream) {
    if (!e || !dev_weights || !dcfp_aligned16(dev_weights)) return DCFP_E_BADDESC;
    const File& f = e->file;
    // the input section starts where the blob, rounded up to 256 bytes, ends: one copy carries both
    const size_t n = f.has_input ? table_offset(e) + kTableBytes : f.weights_size;
    const hipError_t st = hipMemcpyAsync(dev_weights, f.bytes.data() + f.weights_off, n, hipMemcpyHostToDevice, dcfp_s(stream));
    return st == hipSuccess ? DCFP_OK : (int)st;
}

int dcfp_engine_output_shape(dcfp_engine_t e, int N, int H, int W, int* C, int* h, int* w) {
    if (!e || !C || !h || !w) return DCFP_E_BADDESC;
    const Program* P = program(e, N, H, W);
    if (P->status != DCFP_OK) return P->status;
    *C = e->file.meta.num_classes; *h = P->out_h; *w = P->out_w;
    return DCFP_OK;
}

int dcfp_engine_buffer_shapes(dcfp_engine_t e, int H, int W, int* hw_pairs, int n_pairs) {
    if (!e || !hw_pairs || n_pairs < (int)e->file.buffers.size()) return DCFP_E_BADDESC;
    const Program* P = program(e, 1, H, W);
    if (P->status != DCFP_OK) return P->status;
    for (int b = 0; b < n_pairs; ++b) {
        const bool known = b < (int)P->h.size();
        hw_pairs[2 * b] = known ? P->h[b] : 0;
        hw_pairs[2 * b + 1] = known ? P->w[b] : 0;
    }
    return DCFP_OK;
}

size_t dcfp_engine_workspace_bytes(dcfp_engine_t e, int N, int H, int W) {
    if (!e) return 0;
    const Program* P = program(e, N, H, W);
    return P->status == DCFP_OK ? P->total : 0;
}

int dcfp_engine_run_f32(dcfp_engine_t e, const void* dev_weights, const float* image_nchw, int N, int H, int W,
                        void* workspace, size_t workspace_bytes, float* logits_nchw, dcfp_stream_t stream) {
    const Program* P = nullptr;
    int st = check_run(e, dev_weights, image_nchw, N, H, W, workspace, workspace_bytes, logits_nchw, &P);
    if (st != DCFP_OK) return st;
    void* in = static_cast<char*>(workspace) + P->slot_off[e->slot_of[0]];
    st = dcfp_nchw_f32_to_nhwc_f16(image_nchw, in, N, e->file.meta.in_channels, H, W, e->file.buffers[0].pitch, stream);
    if (st != DCFP_OK) return st;
    return run_plan(e, *P, dev_weights, workspace, logits_nchw, dcfp_s(stream));
}

int dcfp_engine_run_u8(dcfp_engine_t e, const void* dev_weights, const uint8_t* image_hwc, size_t row_pitch_bytes, int N,
                       int H, int W, void* workspace, size_t workspace_bytes, float* logits_nchw, dcfp_stream_t stream) {
    if (e && !e->file.has_input) return DCFP_E_UNSUPPORTED;
    const Program* P = nullptr;
    int st = check_run(e, dev_weights, image_hwc, N, H, W, workspace, workspace_bytes, logits_nchw, &P);
    if (st != DCFP_OK) return st;
    if (W > 0 && row_pitch_bytes < 3 * (size_t)W) return DCFP_E_BADDESC;
    void* in = static_cast<char*>(workspace) + P->slot_off[e->slot_of[0]];
    const void* table = static_cast<const char*>(dev_weights) + table_offset(e);
    st = dcfp_image_u8_hwc_to_nhwc_f16(image_hwc, row_pitch_bytes, N, H, W, table, e->file.order, in,
                                       e->file.buffers[0].pitch, stream);
    if (st != DCFP_OK) return st;
    return run_plan(e, *P, dev_weights, workspace, logits_nchw, dcfp_s(stream));
}

}  // extern "C"
