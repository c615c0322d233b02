// ckpt_format.h — the framing of a checkpoint file: pure host code (no HIP), used by iblb_load_checkpoint and
// iblb_checkpoint_info (iblb_ctx.hip) and checked on the CPU by tests/ckpt_format_main.cpp.
//
// A checkpoint is the fluid part (what iblb_save_checkpoint writes; its length follows from its header,
// fluid_bytes below), optionally followed by the observer part (iblb_save_checkpoint_ex):
//
//   fluid part | section* | end section
//
// Every section is a 16-byte section header — an 8-byte tag, then the payload's length in bytes as an int64
// (host byte order, like every number of the file) — followed by that many bytes of payload.  The tags, in the
// only order a file may hold them, each at most once:
//
//   "IBLBSCL1"  the passive scalar with its source, uptake, ends and gauges
//   "IBLBTRC1"  the passive tracers
//   "IBLBAVG1"  the averaged fields
//   "IBLBEND1"  the end section: payload length 0, and nothing behind it
//
// A file that ends with the fluid part holds no observers and is valid.  A file that goes on must go on with
// sections and close with the end section; the end section alone is valid too (no observers).  What the payloads
// hold is described above the checkpoint code of iblb_ctx.hip; nothing here looks into one.
#pragma once

#include <cstdio>
#include <cstring>

namespace iblbck {

constexpr int TAG_BYTES = 8;
constexpr int HEADER_BYTES = 16;  // tag + int64 length
enum Kind { K_SCALAR = 0, K_TRACERS = 1, K_AVERAGE = 2, K_END = 3, N_KINDS = 4 };
constexpr char TAGS[N_KINDS][TAG_BYTES + 1] = {"IBLBSCL1", "IBLBTRC1", "IBLBAVG1", "IBLBEND1"};

struct SectionHeader {
    char tag[TAG_BYTES];
    long long length;  // bytes of payload behind the header
};
static_assert(sizeof(SectionHeader) == HEADER_BYTES, "a section header is 16 bytes");

// ---- the fluid part's header (iblb_save_checkpoint): 8-byte magic, 12 int64, 6 doubles ----
constexpr char FLUID_MAGIC[TAG_BYTES + 1] = "IBLBCK01";
enum { CK_VERSION, CK_NX, CK_NY, CK_XB, CK_NCOL, CK_PREC, CK_T, CK_NS, CK_CILIA, CK_CNUM, CK_CT, CK_CPSTEP, CK_NI };
enum { CK_Q, CK_CSPACE, CK_TAU, CK_TAU2, CK_GX, CK_GY, CK_ND };
constexpr long long FLUID_HEADER_BYTES = TAG_BYTES + 8 * CK_NI + 8 * CK_ND;
constexpr long long SAMPLES_PER_CILIUM = 9600, POINTS_PER_CILIUM = 96;  // per cilium (cilia_kernels.h)

// Bytes of the fluid part whose int64 header fields are iv, or -1 where they cannot be a checkpoint's: the
// header, nine population planes of ncol * ny elements in the storage precision (0: double, 1: float), per
// Lagrangian point two float pairs and an int, and with cilia 7 floats per filament sample and 5 per boundary point.
inline long long fluid_bytes(const long long* iv) {
    const long long lim = 1LL << 40;
    if (iv[CK_VERSION] != 1 || iv[CK_NX] < 1 || iv[CK_NY] < 1 || iv[CK_NCOL] < 1 || iv[CK_NCOL] > iv[CK_NX] ||
        iv[CK_XB] < 0 || iv[CK_XB] > iv[CK_NX] - iv[CK_NCOL] || (iv[CK_PREC] != 0 && iv[CK_PREC] != 1) || iv[CK_T] < 0 ||
        iv[CK_NS] < 0 || iv[CK_NS] > lim || (iv[CK_CILIA] != 0 && iv[CK_CILIA] != 1))
        return -1;
    if (iv[CK_NY] > lim / iv[CK_NCOL]) return -1;
    long long n = FLUID_HEADER_BYTES + 9 * iv[CK_NCOL] * iv[CK_NY] * (iv[CK_PREC] == 0 ? 8 : 4) + 20 * iv[CK_NS];
    if (iv[CK_CILIA]) {
        if (iv[CK_CNUM] < 1 || iv[CK_CNUM] > (1LL << 20)) return -1;
        n += 4 * (7 * SAMPLES_PER_CILIUM + 5 * POINTS_PER_CILIUM) * iv[CK_CNUM];
    }
    return n;
}

// ---- the scanner ----
enum ScanStatus {
    SCAN_OK = 0,
    SCAN_IO,            // the file cannot be sought or read
    SCAN_FLUID_SHORT,   // the file ends inside the fluid part
    SCAN_HEADER_SHORT,  // the file ends inside a section header
    SCAN_TAG,           // a tag that is none of TAGS
    SCAN_ORDER,         // a section out of order or for the second time
    SCAN_LENGTH,        // a negative length, a length running past the end of the file, an end section with a payload
    SCAN_NO_END,        // sections, but the file ends without the end section
    SCAN_TRAILING,      // bytes behind the end section
};

inline const char* scan_message(int status) {
    switch (status) {
        case SCAN_OK: return "ok";
        case SCAN_IO: return "checkpoint: the file cannot be read";
        case SCAN_FLUID_SHORT: return "checkpoint: the file ends inside the fluid part";
        case SCAN_HEADER_SHORT: return "checkpoint: the file ends inside a section header";
        case SCAN_TAG: return "checkpoint: an unknown section tag";
        case SCAN_ORDER: return "checkpoint: a section out of order or given twice";
        case SCAN_LENGTH: return "checkpoint: a section length that is negative or runs past the end of the file";
        case SCAN_NO_END: return "checkpoint: the observer part has no end section";
        case SCAN_TRAILING: return "checkpoint: bytes behind the end section";
    }
    return "checkpoint: unknown scan status";
}

struct Scan {
    bool present[N_KINDS] = {false, false, false, false};  // [K_END]: the file has an observer part
    long long offset[N_KINDS] = {0, 0, 0, 0};              // of the payload, from the start of the file
    long long length[N_KINDS] = {0, 0, 0, 0};              // of the payload
    long long file_bytes = 0;
    unsigned observers() const {  // the IBLB_CKPT_* bits of the sections present
        return (present[K_SCALAR] ? 1u : 0u) | (present[K_TRACERS] ? 2u : 0u) | (present[K_AVERAGE] ? 4u : 0u);
    }
};

// Walks f from fluid_end, the end of the fluid part, to the end section.  Returns a ScanStatus; *out is complete
// only with SCAN_OK.  Reads section headers only; leaves the file position unspecified.
inline int scan(std::FILE* f, long long fluid_end, Scan* out) {
    *out = Scan{};
    if (fluid_end < 0 || std::fseek(f, 0, SEEK_END) != 0) return SCAN_IO;
    const long long size = (long long)std::ftell(f);
    if (size < 0) return SCAN_IO;
    out->file_bytes = size;
    if (size < fluid_end) return SCAN_FLUID_SHORT;
    long long pos = fluid_end;
    int last = -1;  // the kind of the section before this one
    while (pos < size) {
        if (size - pos < HEADER_BYTES) return SCAN_HEADER_SHORT;
        SectionHeader h;
        if (std::fseek(f, (long)pos, SEEK_SET) != 0 || std::fread(&h, HEADER_BYTES, 1, f) != 1) return SCAN_IO;
        int kind = -1;
        for (int k = 0; k < N_KINDS; ++k)
            if (std::memcmp(h.tag, TAGS[k], TAG_BYTES) == 0) kind = k;
        if (kind < 0) return SCAN_TAG;
        if (kind <= last) return SCAN_ORDER;
        pos += HEADER_BYTES;
        if (h.length < 0 || h.length > size - pos || (kind == K_END && h.length != 0)) return SCAN_LENGTH;
        out->present[kind] = true;
        out->offset[kind] = pos;
        out->length[kind] = h.length;
        pos += h.length;
        last = kind;
        if (kind == K_END) return pos == size ? SCAN_OK : SCAN_TRAILING;
    }
    return last < 0 ? SCAN_OK : SCAN_NO_END;
}

// The fluid header of f read and checked as far as a file alone allows: the magic, the version, and fields that
// fluid_bytes accepts.  iv: CK_NI int64, dv: CK_ND doubles.  Returns the fluid part's bytes, or -1.
inline long long read_fluid_header(std::FILE* f, long long* iv, double* dv) {
    char magic[TAG_BYTES];
    if (std::fseek(f, 0, SEEK_SET) != 0 || std::fread(magic, 1, TAG_BYTES, f) != (size_t)TAG_BYTES ||
        std::memcmp(magic, FLUID_MAGIC, TAG_BYTES) != 0)
        return -1;
    if (std::fread(iv, 8, CK_NI, f) != (size_t)CK_NI || std::fread(dv, 8, CK_ND, f) != (size_t)CK_ND) return -1;
    return fluid_bytes(iv);
}

}  // namespace iblbck
