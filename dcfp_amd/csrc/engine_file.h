// engine_file.h — the flat engine file: byte layout and a host-only parser that trusts nothing in the
// file.  Plain C++17, no HIP include: engine_file.cpp compiles with the host compiler alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace dcfp_efile {

// ---- byte layout (little-endian; every integer int32 unless said otherwise)
constexpr char kMagic[8] = {'D', 'C', 'F', 'P', 'E', 'N', 'G', '\0'};
constexpr uint32_t kVersion = 1;
enum Section { SEC_META = 0, SEC_RECORDS, SEC_BUFFERS, SEC_TENSORS, SEC_STRINGS, SEC_WEIGHTS, SEC_INPUT, SEC_COUNT };
// header: magic[8], u32 version, u32 header_bytes, u64 file_bytes, u32 n_sections, u32 0, then {u64 offset, u64 size}
// per section in the order above
constexpr size_t kHeaderFixed = 32, kHeaderBytes = kHeaderFixed + 16 * SEC_COUNT;
constexpr size_t kMetaBytes = 32, kRecordBytes = 136, kBufferBytes = 16, kTensorBytes = 24;
// input section: 3 x 256 fp16, then order[3] and a 0; it starts where the weight blob, rounded up to 256 bytes, ends,
// so that blob and table reach the device in one copy
constexpr size_t kTableHalfs = 3 * 256, kTableBytes = kTableHalfs * 2, kInputBytes = kTableBytes + 16;
constexpr size_t kWeightAlign = 256, kSectionAlign = 16;

// ---- limits a file must stay within
constexpr int kMaxRecords = 4096, kMaxBuffers = 4096, kMaxTensors = 3 * kMaxRecords;
constexpr int kMaxPitch = 1 << 16, kMaxCout = 1 << 16, kMaxPad = 8192, kMaxDil = 4096;
constexpr size_t kMaxStrings = 1 << 20;
constexpr int kPyramidMaxLevels = 4, kPyramidMaxSize = 8;   // PYRAMID_MAX_LEVELS / PYRAMID_MAX_SIZE of deploy.py

enum Op { OP_CONV = 1, OP_MAXPOOL, OP_AVGPOOL, OP_BROADCAST, OP_CAST, OP_RESIZE, OP_PYRAMID, OP_END };
enum Fmt { FMT_F16 = 0, FMT_F8 = 1 };
enum Dtype { DT_F16 = 0, DT_F32 = 1, DT_F8 = 2 };

struct Record {   // one plan entry: the fields Engine._program reads (absent ones 0, absent ids -1)
    int32_t op, name, fmt, src, dst, res;
    int32_t k, stride, pad, dil, cin8, cout, y_off, x_off, c, c8, relu, f32, align, nlev;
    int32_t sizes[4], dsts[4];
    int32_t t_w, t_a, t_b;   // tensor ids: packed weight; shift (fp16) or mul (fp8); add (fp8)
    int32_t reserved;
    float res_mul, scale;    // the exact fp32 the ctypes call of the Python engine passes
};
static_assert(sizeof(Record) == kRecordBytes, "record layout");

struct Buffer {
    int32_t pitch, fmt;
    float scale;
    int32_t reserved;
};
static_assert(sizeof(Buffer) == kBufferBytes, "buffer layout");

struct Tensor {
    int32_t dtype, reserved;
    uint64_t bytes, offset;   // offset into the weight blob, a multiple of 256
};
static_assert(sizeof(Tensor) == kTensorBytes, "tensor layout");

struct Meta {
    int32_t format, align_corner, num_classes, in_channels, model, n_records, n_buffers, n_tensors;
};
static_assert(sizeof(Meta) == kMetaBytes, "meta layout");

struct File {   // a parsed, validated file; `bytes` is the file itself, the offsets point into it
    std::vector<unsigned char> bytes;
    Meta meta{};
    std::vector<Record> records;
    std::vector<Buffer> buffers;
    std::vector<Tensor> tensors;
    size_t strings_off = 0, strings_size = 0;
    size_t weights_off = 0, weights_size = 0;
    bool has_input = false;
    int32_t order[3] = {0, 1, 2};
    size_t table_off = 0;    // 3 x 256 fp16, when has_input
    const char* name(const Record& r) const { return reinterpret_cast<const char*>(bytes.data()) + strings_off + r.name; }
};

// Parses and validates `n` bytes into `out` (which takes a copy).  false: `err` (when given) holds a one-line,
// NUL-terminated message.  Never reads outside [bytes, bytes + n).
bool parse(const void* bytes, size_t n, File& out, char* err, size_t errlen);
// Reads the file at `path`, then parse().
bool load(const char* path, File& out, char* err, size_t errlen);

}  // namespace dcfp_efile
