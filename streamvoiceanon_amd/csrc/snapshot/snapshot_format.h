// Container of one saved stream (sva_stream_save / sva_stream_load).  Host-only and self-contained: no HIP, no engine types, so the parser --
// which takes untrusted bytes -- can be compiled alone under a host sanitizer (tests/test_snapshot_format_cpu.py).
//
// Little-endian, fixed layout:
//     0  char[8]  magic "SVASNAP1"
//     8  u32      format version (kVersion)
//    12  u32      header bytes = offset of the payload (a multiple of 16)
//    16  u64      total bytes = header bytes + payload bytes
//    24  u64      payload bytes (a multiple of 16)
//    32  u64      payload checksum (fnv1a64_words)
//    40  u64      header checksum (fnv1a64 of the header bytes with this field as zeros)
//    48  u32      n_cfg     values of the configuration signature
//    52  u32      n_layout  values of the layout signature
//    56  u32      ref_len   frames of the stored prompt
//    60  u32      ncb       codebooks of the stored prompt's audio codes
//    64  i32 x 6  frames decoded, last_pos, content count, ar_dtype, chunk_frames, 0
//    88  f32 x 4  temperature as set, inv_temp, top_p, 0           (the slot's sampling pair, SlotHost)
//   104  i64[n_cfg] | i64[n_layout] | i64[ref_len] stored content codes | i32[ncb][ref_len] stored audio codes | zeros up to a multiple of 16
//   then the payload: the slot's segments in the order of slot_state.h, each padded to 16 bytes with zeros.
// No timestamps, no pointers, no uninitialised bytes: two saves of an unchanged slot are byte-identical.
// The parser reads nothing past `nbytes` and checks every count it finds against the bytes that are left before it uses it.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

namespace sva {
namespace snap {

constexpr uint32_t kVersion = 1;
constexpr size_t kFixedBytes = 104;
constexpr char kMagic[8] = {'S', 'V', 'A', 'S', 'N', 'A', 'P', '1'};

// refusal codes of the parser and of the comparison against a batch (sva_stream_load / sva_stream_blob_info / sva_test_snapshot_header)
enum Refusal : int {
    kOk = 0,
    kTruncated = -10,        // fewer bytes than the blob says it has (or than a header needs)
    kBadMagic = -11,
    kBadVersion = -12,
    kBadHeader = -13,        // a count or length of the header contradicts another, or the header checksum fails
    kBadChecksum = -14,      // the payload checksum fails
    kConfigMismatch = -15,   // configuration signature differs from the batch's
    kLayoutMismatch = -16,   // layout signature differs from the batch's
    kSizeMismatch = -17,     // payload length is not what the batch's segments hold at the blob's KV position
};

struct Fields {
    int32_t nframes = 0, last_pos = -1, ncontent = 0, ar_dtype = 0, chunk_frames = 1;
    float temperature = 0.7f, inv_temp = 1.0f / 0.7f, top_p = 0.7f;
    int32_t ncb = 0;
    std::vector<int64_t> ref_content;      // [ref_len]
    std::vector<int32_t> ref_audio;        // [ncb][ref_len]
};

struct Header {
    uint32_t version = 0, header_bytes = 0;
    uint64_t total_bytes = 0, payload_bytes = 0, payload_sum = 0;
    std::vector<int64_t> cfg, layout;
    Fields f;
};

inline uint64_t fnv1a64(const uint8_t* p, size_t n, uint64_t h = 0xcbf29ce484222325ull) {
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h;
}
// FNV-1a over little-endian 64-bit words (n a multiple of 8): the payload is up to ~110 MB, a byte at a time would cost ~0.4 s
inline uint64_t fnv1a64_words(const uint8_t* p, size_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i + 8 <= n; i += 8) {
        uint64_t w;
        memcpy(&w, p + i, 8);
#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ == __ORDER_BIG_ENDIAN__
        w = __builtin_bswap64(w);
#endif
        h ^= w;
        h *= 0x100000001b3ull;
    }
    return h;
}

inline void put_u32(uint8_t* p, uint32_t v) { for (int i = 0; i < 4; ++i) p[i] = (uint8_t)(v >> (8 * i)); }
inline void put_u64(uint8_t* p, uint64_t v) { for (int i = 0; i < 8; ++i) p[i] = (uint8_t)(v >> (8 * i)); }
inline uint32_t get_u32(const uint8_t* p) { uint32_t v = 0; for (int i = 0; i < 4; ++i) v |= (uint32_t)p[i] << (8 * i); return v; }
inline uint64_t get_u64(const uint8_t* p) { uint64_t v = 0; for (int i = 0; i < 8; ++i) v |= (uint64_t)p[i] << (8 * i); return v; }
inline void put_f32(uint8_t* p, float f) { uint32_t v; memcpy(&v, &f, 4); put_u32(p, v); }
inline float get_f32(const uint8_t* p) { const uint32_t v = get_u32(p); float f; memcpy(&f, &v, 4); return f; }

// bounds of the counts a header may carry (anything larger is a corrupt header, whatever nbytes is)
constexpr uint64_t kMaxCfg = 4096, kMaxLayout = 1u << 22, kMaxRefLen = 1u << 20, kMaxNcb = 64;

inline uint64_t header_bytes_for(uint64_t n_cfg, uint64_t n_layout, uint64_t ref_len, uint64_t ncb) {
    const uint64_t n = kFixedBytes + 8 * n_cfg + 8 * n_layout + 8 * ref_len + 4 * ncb * ref_len;
    return (n + 15) & ~(uint64_t)15;
}

// the header of a blob whose payload (payload_bytes, checksum payload_sum) follows it: exactly header_bytes_for(...) bytes into dst
inline void write_header(uint8_t* dst, const std::vector<int64_t>& cfg, const std::vector<int64_t>& layout, const Fields& f, uint64_t payload_bytes,
                         uint64_t payload_sum) {
    const uint64_t ref_len = f.ref_content.size();
    const uint64_t hb = header_bytes_for(cfg.size(), layout.size(), ref_len, (uint64_t)f.ncb);
    memset(dst, 0, (size_t)hb);
    memcpy(dst, kMagic, 8);
    put_u32(dst + 8, kVersion);
    put_u32(dst + 12, (uint32_t)hb);
    put_u64(dst + 16, hb + payload_bytes);
    put_u64(dst + 24, payload_bytes);
    put_u64(dst + 32, payload_sum);
    put_u32(dst + 48, (uint32_t)cfg.size());
    put_u32(dst + 52, (uint32_t)layout.size());
    put_u32(dst + 56, (uint32_t)ref_len);
    put_u32(dst + 60, (uint32_t)f.ncb);
    const int32_t ints[6] = {f.nframes, f.last_pos, f.ncontent, f.ar_dtype, f.chunk_frames, 0};
    for (int i = 0; i < 6; ++i) put_u32(dst + 64 + 4 * i, (uint32_t)ints[i]);
    put_f32(dst + 88, f.temperature); put_f32(dst + 92, f.inv_temp); put_f32(dst + 96, f.top_p);
    uint8_t* p = dst + kFixedBytes;
    for (int64_t v : cfg) { put_u64(p, (uint64_t)v); p += 8; }
    for (int64_t v : layout) { put_u64(p, (uint64_t)v); p += 8; }
    for (int64_t v : f.ref_content) { put_u64(p, (uint64_t)v); p += 8; }
    for (size_t i = 0; i < (size_t)f.ncb * ref_len; ++i) { put_u32(p, (uint32_t)(i < f.ref_audio.size() ? f.ref_audio[i] : 0)); p += 4; }
    put_u64(dst + 40, fnv1a64(dst, (size_t)hb));
}

// Parses and validates `nbytes` untrusted bytes.  check_payload: also verify the payload checksum.  Fills *h only on kOk.
inline int parse(const void* blob, long nbytes, bool check_payload, Header* h) {
    const uint8_t* p = static_cast<const uint8_t*>(blob);
    if (!p || nbytes < 0) return kTruncated;
    const uint64_t n = (uint64_t)nbytes;
    if (n < 8) return kTruncated;
    if (memcmp(p, kMagic, 8) != 0) return kBadMagic;
    if (n < 12) return kTruncated;
    const uint32_t version = get_u32(p + 8);
    if (version != kVersion) return kBadVersion;
    if (n < kFixedBytes) return kTruncated;
    const uint64_t hb = get_u32(p + 12), total = get_u64(p + 16), payload = get_u64(p + 24);
    const uint64_t n_cfg = get_u32(p + 48), n_layout = get_u32(p + 52), ref_len = get_u32(p + 56), ncb = get_u32(p + 60);
    if (n_cfg > kMaxCfg || n_layout > kMaxLayout || ref_len > kMaxRefLen || ncb > kMaxNcb) return kBadHeader;
    if (hb != header_bytes_for(n_cfg, n_layout, ref_len, ncb)) return kBadHeader;
    if (payload % 16 != 0 || payload > ((uint64_t)1 << 40) || total != hb + payload) return kBadHeader;
    if (n < hb) return kTruncated;
    {   // header checksum, its own field read as zeros
        uint64_t s = fnv1a64(p, 40);
        const uint8_t zeros[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        s = fnv1a64(zeros, 8, s);
        s = fnv1a64(p + 48, (size_t)hb - 48, s);
        if (s != get_u64(p + 40)) return kBadHeader;
    }
    if (n < total) return kTruncated;
    if (n > total) return kBadHeader;
    const uint64_t sum = get_u64(p + 32);
    if (check_payload && fnv1a64_words(p + hb, (size_t)payload) != sum) return kBadChecksum;
    if (!h) return kOk;
    h->version = version; h->header_bytes = (uint32_t)hb; h->total_bytes = total; h->payload_bytes = payload; h->payload_sum = sum;
    Fields& f = h->f;
    f.nframes = (int32_t)get_u32(p + 64); f.last_pos = (int32_t)get_u32(p + 68); f.ncontent = (int32_t)get_u32(p + 72);
    f.ar_dtype = (int32_t)get_u32(p + 76); f.chunk_frames = (int32_t)get_u32(p + 80);
    f.temperature = get_f32(p + 88); f.inv_temp = get_f32(p + 92); f.top_p = get_f32(p + 96);
    f.ncb = (int32_t)ncb;
    const uint8_t* q = p + kFixedBytes;
    h->cfg.resize((size_t)n_cfg); h->layout.resize((size_t)n_layout); f.ref_content.resize((size_t)ref_len); f.ref_audio.resize((size_t)(ncb * ref_len));
    for (auto& v : h->cfg) { v = (int64_t)get_u64(q); q += 8; }
    for (auto& v : h->layout) { v = (int64_t)get_u64(q); q += 8; }
    for (auto& v : f.ref_content) { v = (int64_t)get_u64(q); q += 8; }
    for (auto& v : f.ref_audio) { v = (int32_t)get_u32(q); q += 4; }
    return kOk;
}

// index of the first value in which two signatures differ (their common length if only the lengths differ), -1: equal
inline long first_difference(const std::vector<int64_t>& a, const std::vector<int64_t>& b) {
    const size_t n = a.size() < b.size() ? a.size() : b.size();
    for (size_t i = 0; i < n; ++i)
        if (a[i] != b[i]) return (long)i;
    return a.size() == b.size() ? -1 : (long)n;
}

// a parsed header against a batch's signatures: kOk, kConfigMismatch or kLayoutMismatch; *field = index of the first differing value
inline int compare(const Header& h, const std::vector<int64_t>& cfg, const std::vector<int64_t>& layout, long* field) {
    long d = first_difference(h.cfg, cfg);
    if (d >= 0) { if (field) *field = d; return kConfigMismatch; }
    d = first_difference(h.layout, layout);
    if (d >= 0) { if (field) *field = d; return kLayoutMismatch; }
    if (field) *field = -1;
    return kOk;
}

}  // namespace snap
}  // namespace sva
