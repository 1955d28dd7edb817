// Test hooks of the snapshot code (include/sva.h): the pack / unpack kernels alone on a synthetic arena, and the container's builder, parser
// and signature comparison without a device.  Nothing of an engine is involved.
#include "slot_pack.h"
#include "snapshot_format.h"

#include <string.h>

using namespace sva;

namespace {
struct HookBuf {
    void* p = nullptr;
    HookBuf() = default;
    HookBuf(const HookBuf&) = delete;
    HookBuf& operator=(const HookBuf&) = delete;
    ~HookBuf() { if (p) (void)hipFree(p); }
    int put(const void* host, size_t bytes) {
        SVA_HIP(hipMalloc(&p, bytes ? bytes : 16));
        if (bytes) SVA_HIP(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
        return 0;
    }
};
}  // namespace

extern "C" int sva_test_slot_pack(int device, const long* table, int n_seg, const void* arena_src, long src_bytes, void* arena_dst, long dst_bytes, int slot_src,
                                  int slot_dst, int step_src, int step_dst, void* image_out, long image_bytes, int cus) {
    SVA_CHECK(table && arena_src && arena_dst && image_out && n_seg >= 1 && n_seg <= 4096, "slot_pack hook: null argument or segment count");
    SVA_CHECK(src_bytes >= 1 && dst_bytes >= 1 && slot_src >= 0 && slot_dst >= 0 && step_src >= 0 && step_dst >= 0 && cus >= 1 && cus <= 1024, "slot_pack hook: bad arguments");
    SVA_HIP(hipSetDevice(device));
    HookBuf src, dst, img, tab_s, tab_d, steps;
    SVA_TRY(src.put(arena_src, (size_t)src_bytes));
    SVA_TRY(dst.put(arena_dst, (size_t)dst_bytes));
    SlotSegments Ls, Ld;
    for (int i = 0; i < n_seg; ++i) {
        const long* t = table + 9L * i;
        const long off_s = t[0], off_d = t[1], slot_stride = t[2], row_stride = t[3], row_bytes = t[4], rows = t[5], kind = t[6], elem = t[7], ring_step = t[8];
        SVA_CHECK(off_s >= 0 && off_d >= 0 && slot_stride >= 0 && rows >= 0 && rows <= (1 << 20) && row_bytes >= 1 && row_stride >= row_bytes &&
                      (elem == 2 || elem == 4) && kind >= 0 && kind <= 3 && ring_step >= 0 && ring_step <= (1 << 24),
                  "slot_pack hook: bad segment");
        // every byte the kernels may touch lies inside the arenas
        const long span = rows ? (rows - 1) * row_stride + row_bytes : 0;
        SVA_CHECK(off_s + slot_src * slot_stride + span <= src_bytes, "slot_pack hook: a segment leaves the source arena");
        SVA_CHECK(off_d + slot_dst * slot_stride + span <= dst_bytes, "slot_pack hook: a segment leaves the destination arena");
        Ls.add("s", static_cast<char*>(src.p) + off_s, slot_stride, (int)rows, row_bytes, row_stride, (int)kind, (int)elem, (int)ring_step);
        Ld.add("d", static_cast<char*>(dst.p) + off_d, slot_stride, (int)rows, row_bytes, row_stride, (int)kind, (int)elem, (int)ring_step);
    }
    SVA_TRY(check_slot_segments(Ls));
    SVA_TRY(check_slot_segments(Ld));
    SVA_CHECK(Ls.image_bytes == image_bytes, "slot_pack hook: image_bytes is not the sum of the padded segment lengths");
    std::vector<unsigned char> fill((size_t)image_bytes, 0xA5);          // the pack must write every byte, padding included
    SVA_TRY(img.put(fill.data(), fill.size()));
    SVA_TRY(tab_s.put(Ls.seg.data(), sizeof(SlotSegment) * Ls.seg.size()));
    SVA_TRY(tab_d.put(Ld.seg.data(), sizeof(SlotSegment) * Ld.seg.size()));
    const int st[2] = {step_src, step_dst};
    SVA_TRY(steps.put(st, sizeof(st)));
    SVA_TRY(launch_slot_pack(static_cast<const SlotSegment*>(tab_s.p), n_seg, slot_src, static_cast<const int*>(steps.p), img.p, image_bytes, cus, 0));
    SVA_HIP(hipDeviceSynchronize());
    SVA_HIP(hipMemcpy(image_out, img.p, (size_t)image_bytes, hipMemcpyDeviceToHost));
    SVA_TRY(launch_slot_unpack(static_cast<const SlotSegment*>(tab_d.p), n_seg, slot_dst, static_cast<const int*>(steps.p) + 1, img.p, image_bytes, cus, 0));
    SVA_HIP(hipDeviceSynchronize());
    SVA_HIP(hipMemcpy(arena_dst, dst.p, (size_t)dst_bytes, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int sva_test_snapshot_header(int op, const long* desc, const long* sig, const void* bytes, long nbytes, void* out, long out_cap, long* result) {
    SVA_CHECK(desc && result && (op == 0 || op == 1), "snapshot_header hook: null argument or unknown op");
    const long n_cfg = desc[0], n_layout = desc[1];
    SVA_CHECK(n_cfg >= 0 && n_cfg <= 4096 && n_layout >= 0 && n_layout <= 65536 && (sig || n_cfg + n_layout == 0), "snapshot_header hook: signature lengths");
    std::vector<int64_t> cfg(sig, sig + n_cfg), layout(sig + n_cfg, sig + n_cfg + n_layout);
    for (int i = 0; i < 12; ++i) result[i] = -1;
    if (op == 0) {          // build: desc = {n_cfg, n_layout, nframes, last_pos, ncontent, ar_dtype, chunk_frames, ncb, ref_len}; sig continues with the stored prompt
        snap::Fields f;
        f.nframes = (int)desc[2]; f.last_pos = (int)desc[3]; f.ncontent = (int)desc[4]; f.ar_dtype = (int)desc[5]; f.chunk_frames = (int)desc[6];
        f.ncb = (int)desc[7];
        const long ref_len = desc[8];
        SVA_CHECK(f.ncb >= 0 && f.ncb <= 64 && ref_len >= 0 && ref_len <= 4096, "snapshot_header hook: stored prompt");
        SVA_CHECK(nbytes >= 0 && nbytes % 16 == 0 && (bytes || nbytes == 0) && out, "snapshot_header hook: the payload is a multiple of 16 bytes");
        const long* pr = sig + n_cfg + n_layout;
        f.ref_content.assign(pr, pr + ref_len);
        for (long i = 0; i < (long)f.ncb * ref_len; ++i) f.ref_audio.push_back((int32_t)pr[ref_len + i]);
        const long hb = (long)snap::header_bytes_for((uint64_t)n_cfg, (uint64_t)n_layout, (uint64_t)ref_len, (uint64_t)f.ncb);
        result[0] = hb + nbytes;
        SVA_CHECK(out_cap >= hb + nbytes, "snapshot_header hook: output buffer too small");
        uint8_t* o = static_cast<uint8_t*>(out);
        if (nbytes) memcpy(o + hb, bytes, (size_t)nbytes);
        snap::write_header(o, cfg, layout, f, (uint64_t)nbytes, snap::fnv1a64_words(o + hb, (size_t)nbytes));
        return 0;
    }
    // check: `bytes` against the scripted batch (sig = its two signatures, desc[2] = the payload bytes its segments hold, < 0: not compared)
    // result = {refusal code, first differing field, version, frames, last_pos, content count, ref_len, ar_dtype, chunk_frames, payload bytes, ncb, header bytes}
    snap::Header h;
    int rc = snap::parse(bytes, nbytes, true, &h);
    long field = -1;
    if (!rc) {
        result[2] = h.version; result[3] = h.f.nframes; result[4] = h.f.last_pos; result[5] = h.f.ncontent; result[6] = (long)h.f.ref_content.size();
        result[7] = h.f.ar_dtype; result[8] = h.f.chunk_frames; result[9] = (long)h.payload_bytes; result[10] = h.f.ncb; result[11] = h.header_bytes;
        rc = snap::compare(h, cfg, layout, &field);
        if (!rc && desc[2] >= 0 && (long)h.payload_bytes != desc[2]) rc = snap::kSizeMismatch;
    }
    result[0] = rc; result[1] = field;
    return 0;
}
