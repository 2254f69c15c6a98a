// engine_file.cpp — parser of the flat engine file.  Host only.  Every offset, count, id and size in the
// file is checked before it is used; a bad file gives `false` and a one-line message, never a read out of bounds.
// (The layout is little-endian and so is every host this library is built for: the tables are copied out with memcpy.)
#include "engine_file.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

namespace dcfp_efile {
namespace {

bool fail(char* err, size_t errlen, const char* fmt, ...) {
    if (err && errlen) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, errlen, fmt, ap);
        va_end(ap);
    }
    return false;
}

uint32_t rd32(const unsigned char* p) { uint32_t v; memcpy(&v, p, 4); return v; }
uint64_t rd64(const unsigned char* p) { uint64_t v; memcpy(&v, p, 8); return v; }

int64_t round_up(int64_t v, int g) { return (v + g - 1) / g * g; }
int gran(int fmt) { return fmt == FMT_F8 ? 16 : 8; }
bool is01(int v) { return v == 0 || v == 1; }

struct Checker {
    const File& f;
    char* err;
    size_t errlen;
    const char* name = "";
    int index = 0;

    bool bad(const char* what) const { return fail(err, errlen, "engine file: record %d (%s): %s", index, name, what); }
    bool buffer_id(int b) const { return b >= 0 && b < (int)f.buffers.size(); }
    // tensor `t` exists, has dtype `dt` and exactly `bytes` bytes
    bool tensor(int t, int dt, int64_t bytes, const char* what) const {
        if (t < 0 || t >= (int)f.tensors.size()) return bad(what);
        const Tensor& x = f.tensors[t];
        if (x.dtype != dt || x.bytes != (uint64_t)bytes) return bad(what);
        return true;
    }
    // channels [off, off + width) are a granule-aligned slice of buffer b
    bool slice(int b, int64_t off, int64_t width) const {
        const int g = gran(f.buffers[b].fmt);
        return off >= 0 && off % g == 0 && width > 0 && off + width <= f.buffers[b].pitch;
    }
};

bool check_record(Checker& ck, const Record& r, std::vector<char>& defined, int& classifiers) {
    const File& f = ck.f;
    if (r.op < OP_CONV || r.op >= OP_END) return ck.bad("unknown op code");
    if (r.fmt != FMT_F16 && r.fmt != FMT_F8) return ck.bad("unknown storage format");
    if (f.meta.format == 1 && r.fmt != FMT_F16) return ck.bad("an fp8 record in a format-1 engine");
    if (r.reserved != 0) return ck.bad("reserved field is not 0");
    if (!ck.buffer_id(r.src)) return ck.bad("source buffer id out of range");
    if (!defined[r.src]) return ck.bad("reads a buffer no earlier record wrote");
    const bool f32 = r.op == OP_CONV && r.f32 == 1;
    if (f32 ? r.dst != -1 : !ck.buffer_id(r.dst)) return ck.bad("destination buffer id out of range");
    if (r.op == OP_CONV && r.res != -1) {
        if (!ck.buffer_id(r.res)) return ck.bad("residual buffer id out of range");
        if (!defined[r.res]) return ck.bad("adds a buffer no earlier record wrote");
    } else if (r.res != -1) {
        return ck.bad("a residual on a record that is no conv");
    }
    const Buffer& src = f.buffers[r.src];
    const Buffer* dst = f32 ? nullptr : &f.buffers[r.dst];
    if (r.y_off < 0) return ck.bad("negative channel offset");
    switch (r.op) {
    case OP_CONV: {
        if (r.k != 1 && r.k != 3) return ck.bad("filter size is not 1 or 3");
        if (r.stride != 1 && r.stride != 2) return ck.bad("stride is not 1 or 2");
        if (r.pad < 0 || r.pad > kMaxPad || r.dil < 1 || r.dil > kMaxDil) return ck.bad("padding or dilation out of range");
        if (!is01(r.relu) || !is01(r.f32)) return ck.bad("a flag is not 0 or 1");
        if (r.fmt != src.fmt) return ck.bad("record format differs from its source buffer's");
        const int g = gran(r.fmt);
        if (r.cin8 <= 0 || r.cin8 % g || r.cin8 > src.pitch) return ck.bad("cin8 does not fit the source buffer");
        if (r.cout < 1 || r.cout > kMaxCout) return ck.bad("cout out of range");
        const int64_t rows = round_up(r.cout, 8), wide = round_up(r.cout, g);
        if (f32) {
            if (r.res != -1 || r.relu) return ck.bad("the classifier takes no residual and no ReLU");
            if (r.cout != f.meta.num_classes) return ck.bad("the classifier's cout is not num_classes");
            ++classifiers;
        } else {
            if (dst->fmt != r.fmt) return ck.bad("record format differs from its destination buffer's");
            if (!ck.slice(r.dst, r.y_off, wide)) return ck.bad("output slice does not fit the destination buffer");
            if (r.res != -1 && (f.buffers[r.res].fmt != r.fmt || f.buffers[r.res].pitch < wide))
                return ck.bad("residual buffer does not hold the output's channels");
        }
        const int64_t welems = rows * r.k * r.k * r.cin8;
        if (r.fmt == FMT_F16) {
            if (!ck.tensor(r.t_w, DT_F16, welems * 2, "packed weight: wrong id, dtype or size")) return false;
            if (!ck.tensor(r.t_a, DT_F32, rows * 4, "shift: wrong id, dtype or size")) return false;
            if (r.t_b != -1) return ck.bad("an fp16 conv has no third tensor");
        } else {
            if (!ck.tensor(r.t_w, DT_F8, welems, "packed weight: wrong id, dtype or size")) return false;
            if (!ck.tensor(r.t_a, DT_F32, rows * 4, "mul: wrong id, dtype or size")) return false;
            if (!ck.tensor(r.t_b, DT_F32, rows * 4, "add: wrong id, dtype or size")) return false;
        }
        break;
    }
    case OP_MAXPOOL:
        if (r.fmt != src.fmt || r.fmt != dst->fmt) return ck.bad("pool buffers differ in format");
        if (dst->pitch < src.pitch) return ck.bad("destination pitch below the source's");
        break;
    case OP_AVGPOOL:
        if (src.fmt != r.fmt || dst->fmt != FMT_F16) return ck.bad("average pool: wrong buffer formats");
        if (dst->pitch < src.pitch) return ck.bad("destination pitch below the source's");
        break;
    case OP_BROADCAST:
        if (!defined[r.dst]) return ck.bad("writes a buffer of unknown size");
        if (src.fmt != FMT_F16 || dst->fmt != r.fmt) return ck.bad("broadcast: wrong buffer formats");
        if (r.fmt == FMT_F16) {
            if (!ck.slice(r.dst, r.y_off, src.pitch)) return ck.bad("output slice does not fit the destination buffer");
        } else {
            if (r.c < 1 || round_up(r.c, 8) > src.pitch) return ck.bad("channel count does not fit the source buffer");
            if (!ck.slice(r.dst, r.y_off, round_up(r.c, 16))) return ck.bad("output slice does not fit the destination buffer");
        }
        break;
    case OP_CAST:
        if (r.fmt != FMT_F8 || src.fmt != FMT_F16 || dst->fmt != FMT_F8) return ck.bad("cast: wrong buffer formats");
        if (r.c < 1 || round_up(r.c, 8) > src.pitch) return ck.bad("channel count does not fit the source buffer");
        if (!ck.slice(r.dst, r.y_off, round_up(r.c, 16))) return ck.bad("output slice does not fit the destination buffer");
        break;
    case OP_RESIZE:
        if (!defined[r.dst]) return ck.bad("writes a buffer of unknown size");
        if (r.fmt != FMT_F16 || src.fmt != FMT_F16 || dst->fmt != FMT_F16) return ck.bad("resize: wrong buffer formats");
        if (!is01(r.align)) return ck.bad("a flag is not 0 or 1");
        if (!ck.slice(r.dst, r.y_off, src.pitch)) return ck.bad("output slice does not fit the destination buffer");
        break;
    case OP_PYRAMID:
        if (r.fmt != FMT_F16 || src.fmt != FMT_F16) return ck.bad("pyramid: wrong buffer formats");
        if (r.nlev < 1 || r.nlev > kPyramidMaxLevels) return ck.bad("pyramid level count out of range");
        if (r.c8 <= 0 || r.c8 % 8 || r.x_off < 0 || r.x_off % 8 || (int64_t)r.x_off + r.c8 > src.pitch)
            return ck.bad("input slice does not fit the source buffer");
        for (int l = 0; l < r.nlev; ++l) {
            if (r.sizes[l] < 1 || r.sizes[l] > kPyramidMaxSize) return ck.bad("pyramid size out of range");
            if (!ck.buffer_id(r.dsts[l])) return ck.bad("level buffer id out of range");
            if (f.buffers[r.dsts[l]].fmt != FMT_F16 || f.buffers[r.dsts[l]].pitch < r.c8)
                return ck.bad("level buffer does not hold the pooled channels");
            for (int m = 0; m < l; ++m)
                if (r.dsts[m] == r.dsts[l]) return ck.bad("two levels write one buffer");
        }
        if (r.dst != r.dsts[0]) return ck.bad("dst is not the first level's buffer");
        for (int l = 0; l < r.nlev; ++l) defined[r.dsts[l]] = 1;
        break;
    }
    if (!f32) defined[r.dst] = 1;
    return true;
}

}  // namespace

bool parse(const void* bytes, size_t n, File& out, char* err, size_t errlen) {
    if (!bytes) return fail(err, errlen, "engine file: null pointer");
    if (n < kHeaderBytes) return fail(err, errlen, "engine file: %zu bytes is shorter than the header", n);
    const unsigned char* p = static_cast<const unsigned char*>(bytes);
    if (memcmp(p, kMagic, sizeof(kMagic)) != 0) return fail(err, errlen, "engine file: bad magic");
    if (rd32(p + 8) != kVersion)
        return fail(err, errlen, "engine file: version %u (this build reads version %u)", rd32(p + 8), kVersion);
    if (rd32(p + 12) != kHeaderBytes) return fail(err, errlen, "engine file: header size %u", rd32(p + 12));
    if (rd64(p + 16) != (uint64_t)n)
        return fail(err, errlen, "engine file: header says %llu bytes, the file has %zu", (unsigned long long)rd64(p + 16), n);
    if (rd32(p + 24) != SEC_COUNT || rd32(p + 28) != 0) return fail(err, errlen, "engine file: bad section count");
    static const char* const kNames[SEC_COUNT] = {"meta", "records", "buffers", "tensors", "strings", "weights", "input"};
    size_t off[SEC_COUNT], size[SEC_COUNT], end = kHeaderBytes;
    for (int s = 0; s < SEC_COUNT; ++s) {
        const uint64_t o = rd64(p + kHeaderFixed + 16 * s), z = rd64(p + kHeaderFixed + 16 * s + 8);
        if (o > n || z > n - o) return fail(err, errlen, "engine file: section %s runs past the end of the file", kNames[s]);
        if (o % (s == SEC_WEIGHTS ? kWeightAlign : kSectionAlign)) return fail(err, errlen, "engine file: section %s is misaligned", kNames[s]);
        if (o < end) return fail(err, errlen, "engine file: section %s overlaps what precedes it", kNames[s]);
        off[s] = (size_t)o; size[s] = (size_t)z; end = off[s] + size[s];
    }
    File f;
    if (size[SEC_META] != kMetaBytes) return fail(err, errlen, "engine file: meta section has %zu bytes", size[SEC_META]);
    memcpy(&f.meta, p + off[SEC_META], kMetaBytes);
    const Meta& m = f.meta;
    if (m.format != 1 && m.format != 2) return fail(err, errlen, "engine file: engine format %d", m.format);
    if (!is01(m.align_corner)) return fail(err, errlen, "engine file: align_corner %d", m.align_corner);
    if (m.model < 0 || m.model > 3) return fail(err, errlen, "engine file: model kind %d", m.model);
    if (m.num_classes < 1 || m.num_classes > kMaxCout) return fail(err, errlen, "engine file: num_classes %d", m.num_classes);
    if (m.n_records < 1 || m.n_records > kMaxRecords) return fail(err, errlen, "engine file: %d records", m.n_records);
    if (m.n_buffers < 1 || m.n_buffers > kMaxBuffers) return fail(err, errlen, "engine file: %d buffers", m.n_buffers);
    if (m.n_tensors < 1 || m.n_tensors > kMaxTensors) return fail(err, errlen, "engine file: %d tensors", m.n_tensors);
    if (size[SEC_RECORDS] != (size_t)m.n_records * kRecordBytes) return fail(err, errlen, "engine file: record section size");
    if (size[SEC_BUFFERS] != (size_t)m.n_buffers * kBufferBytes) return fail(err, errlen, "engine file: buffer section size");
    if (size[SEC_TENSORS] != (size_t)m.n_tensors * kTensorBytes) return fail(err, errlen, "engine file: tensor section size");
    if (size[SEC_STRINGS] < 1 || size[SEC_STRINGS] > kMaxStrings || p[off[SEC_STRINGS] + size[SEC_STRINGS] - 1] != 0)
        return fail(err, errlen, "engine file: string table is empty, too long or not terminated");
    if (size[SEC_INPUT] != 0 && size[SEC_INPUT] != kInputBytes) return fail(err, errlen, "engine file: input table size");
    f.strings_off = off[SEC_STRINGS]; f.strings_size = size[SEC_STRINGS];
    f.weights_off = off[SEC_WEIGHTS]; f.weights_size = size[SEC_WEIGHTS];

    f.buffers.resize(m.n_buffers);
    memcpy(f.buffers.data(), p + off[SEC_BUFFERS], size[SEC_BUFFERS]);
    for (int b = 0; b < m.n_buffers; ++b) {
        const Buffer& B = f.buffers[b];
        if ((B.fmt != FMT_F16 && B.fmt != FMT_F8) || (m.format == 1 && B.fmt != FMT_F16) || B.reserved != 0)
            return fail(err, errlen, "engine file: buffer %d: bad storage format", b);
        if (B.pitch < 1 || B.pitch > kMaxPitch || B.pitch % gran(B.fmt))
            return fail(err, errlen, "engine file: buffer %d: pitch %d", b, B.pitch);
    }
    if (f.buffers[0].fmt != FMT_F16 || m.in_channels < 1 || m.in_channels > f.buffers[0].pitch)
        return fail(err, errlen, "engine file: in_channels %d does not fit the input buffer", m.in_channels);

    f.tensors.resize(m.n_tensors);
    memcpy(f.tensors.data(), p + off[SEC_TENSORS], size[SEC_TENSORS]);
    uint64_t tend = 0;
    for (int t = 0; t < m.n_tensors; ++t) {
        const Tensor& T = f.tensors[t];
        if (T.dtype < DT_F16 || T.dtype > DT_F8 || T.reserved != 0) return fail(err, errlen, "engine file: tensor %d: dtype", t);
        if (T.offset % kWeightAlign || T.offset < tend || T.offset > f.weights_size || T.bytes > f.weights_size - T.offset)
            return fail(err, errlen, "engine file: tensor %d: offset or size outside the weight blob", t);
        tend = T.offset + T.bytes;
    }

    if (size[SEC_INPUT]) {
        if (off[SEC_INPUT] != off[SEC_WEIGHTS] + (size[SEC_WEIGHTS] + kWeightAlign - 1) / kWeightAlign * kWeightAlign)
            return fail(err, errlen, "engine file: the input table does not follow the weight blob");
        const unsigned char* q = p + off[SEC_INPUT] + kTableBytes;
        for (int c = 0; c < 3; ++c) {
            f.order[c] = (int32_t)rd32(q + 4 * c);
            if (f.order[c] < 0 || f.order[c] > 2) return fail(err, errlen, "engine file: input channel order %d", f.order[c]);
        }
        if (rd32(q + 12) != 0 || m.in_channels != 3) return fail(err, errlen, "engine file: input table on a non-RGB engine");
        f.has_input = true;
        f.table_off = off[SEC_INPUT];
    }

    f.records.resize(m.n_records);
    memcpy(f.records.data(), p + off[SEC_RECORDS], size[SEC_RECORDS]);
    std::vector<char> defined(m.n_buffers, 0);
    defined[0] = 1;
    int classifiers = 0;
    Checker ck{f, err, errlen};
    for (int i = 0; i < m.n_records; ++i) {
        const Record& r = f.records[i];
        if (r.name < 0 || (size_t)r.name >= f.strings_size) return fail(err, errlen, "engine file: record %d: name offset", i);
        ck.index = i;
        ck.name = reinterpret_cast<const char*>(p) + f.strings_off + r.name;   // (terminated: the table ends in NUL)
        if (!check_record(ck, r, defined, classifiers)) return false;
    }
    const Record& last = f.records.back();
    if (classifiers != 1 || last.op != OP_CONV || last.f32 != 1)
        return fail(err, errlen, "engine file: %d fp32 classifier records (exactly one, the last record, is needed)", classifiers);
    f.bytes.assign(p, p + n);
    out = std::move(f);
    return true;
}

bool load(const char* path, File& out, char* err, size_t errlen) {
    if (!path) return fail(err, errlen, "engine file: null path");
    FILE* fp = fopen(path, "rb");
    if (!fp) return fail(err, errlen, "engine file: cannot open %s", path);
    std::vector<unsigned char> buf;
    unsigned char chunk[1 << 16];
    size_t got;
    while ((got = fread(chunk, 1, sizeof(chunk), fp)) > 0) buf.insert(buf.end(), chunk, chunk + got);
    const bool bad = ferror(fp) != 0;
    fclose(fp);
    if (bad) return fail(err, errlen, "engine file: error reading %s", path);
    return parse(buf.data(), buf.size(), out, err, errlen);
}

}  // namespace dcfp_efile
