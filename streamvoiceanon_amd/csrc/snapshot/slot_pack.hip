// slot_pack_kernel / slot_unpack_kernel: every segment of one slot (slot_state.h) between the live buffers of a batch and one contiguous
// device image, in one launch each, driven by a segment table in device memory.
//
// Work is dealt by IMAGE BYTES, not by segment: the KV prefix is > 95 % of an image (288 segments of 64 KB and more) while the ShiftDesc
// histories are hundreds of pieces of a few KB, so a workgroup per segment would leave the chip to 288 workgroups.  Workgroup g owns the
// image bytes [g * per_block, (g + 1) * per_block), per_block a multiple of 4 KB; its 256 lanes sweep that range 16 bytes each per pass,
// so consecutive lanes touch consecutive 16-byte pieces of the image and -- inside a segment -- of the live rows.  A lane finds its segment by
// binary search over the table's img_off once and walks forward from there (its next piece is 4 KB further on).
// A 16-byte piece moves as one uint4 where it lies inside the payload, inside one row (or one run of contiguous rows), does not wrap a ring and
// the live address is 16-byte aligned; otherwise element by element (2 or 4 bytes: fp16 KV rows and unsigned short planes are 2-byte
// elements), which also writes the zero padding behind a segment when packing.  Plain vector loads and stores only.
#include "slot_pack.h"

namespace sva {

namespace {

// last segment whose image starts at or before byte `off` (segments with no rows share their offset with the next one: the last wins)
__device__ __forceinline__ int find_segment(const SlotSegment* __restrict__ segs, int n_seg, long off) {
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].img_off <= off) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <int E> struct ElemT;
template <> struct ElemT<2> { typedef unsigned short type; };
template <> struct ElemT<4> { typedef unsigned int type; };

// byte offset inside the slot's rows of payload byte `rel` of segment g (origin: the ring origin in bytes, 0 for the other kinds)
__device__ __forceinline__ long live_offset(const SlotSegment& g, long rel, long origin) {
    if (g.kind == kSegRing) {
        long pos = origin + rel;
        if (pos >= g.row_bytes) pos -= g.row_bytes;
        return pos;
    }
    if (g.row_stride == g.row_bytes) return rel;
    const long row = rel / g.row_bytes;
    return row * g.row_stride + (rel - row * g.row_bytes);
}

template <bool PACK, int E>
__device__ __forceinline__ void move_elements(const SlotSegment& g, char* live, char* img, long rel, long payload, long origin) {
    typedef typename ElemT<E>::type T;
#pragma unroll
    for (int e = 0; e < 16 / E; ++e) {
        const long r = rel + (long)e * E;
        T* ip = reinterpret_cast<T*>(img + (long)e * E);
        if (r < payload) {
            T* lp = reinterpret_cast<T*>(live + live_offset(g, r, origin));
            if (PACK) *ip = *lp; else *lp = *ip;
        } else if (PACK) {
            *ip = 0;
        }
    }
}

template <bool PACK>
__device__ __forceinline__ void slot_move(const SlotSegment* __restrict__ segs, int n_seg, int slot, const int* __restrict__ step, char* image,
                                          long image_bytes, long per_block) {
    const long lo = (long)blockIdx.x * per_block;
    const long hi = lo + per_block < image_bytes ? lo + per_block : image_bytes;
    long o = lo + (long)threadIdx.x * 16;
    if (o >= hi) return;
    int cur = find_segment(segs, n_seg, o);
    SlotSegment g = segs[cur];
    long next_off = cur + 1 < n_seg ? segs[cur + 1].img_off : image_bytes;
    const long step_now = step ? (long)*step : 0;
    for (; o < hi; o += 256 * 16) {
        if (o >= next_off) {
            int hops = 0;
            while (cur + 1 < n_seg && segs[cur + 1].img_off <= o) {
                if (++hops > 8) { cur = find_segment(segs, n_seg, o); break; }
                ++cur;
            }
            g = segs[cur];
            next_off = cur + 1 < n_seg ? segs[cur + 1].img_off : image_bytes;
        }
        const long rel = o - g.img_off;
        const long payload = (long)g.rows * g.row_bytes;
        char* img = image + o;
        if (rel >= payload) {                  // padding only
            if (PACK) *reinterpret_cast<uint4*>(img) = make_uint4(0, 0, 0, 0);
            continue;
        }
        char* live = g.base + (long)slot * g.slot_stride;
        long origin = 0;
        if (g.kind == kSegRing) origin = ((step_now * g.ring_step) % (g.row_bytes / g.elem)) * g.elem;
        bool wide = rel + 16 <= payload;
        long off = 0;
        if (wide) {
            off = live_offset(g, rel, origin);
            if (g.kind == kSegRing) wide = off + 16 <= g.row_bytes;
            else if (g.row_stride != g.row_bytes) wide = (rel % g.row_bytes) + 16 <= g.row_bytes;
            wide = wide && ((reinterpret_cast<uintptr_t>(live + off) & 15) == 0);
        }
        if (wide) {
            uint4* lp = reinterpret_cast<uint4*>(live + off);
            uint4* ip = reinterpret_cast<uint4*>(img);
            if (PACK) *ip = *lp; else *lp = *ip;
        } else if (g.elem == 2) {
            move_elements<PACK, 2>(g, live, img, rel, payload, origin);
        } else {
            move_elements<PACK, 4>(g, live, img, rel, payload, origin);
        }
    }
}

__global__ __launch_bounds__(256) void slot_pack_kernel(const SlotSegment* __restrict__ segs, int n_seg, int slot, const int* __restrict__ step,
                                                        char* image, long image_bytes, long per_block) {
    slot_move<true>(segs, n_seg, slot, step, image, image_bytes, per_block);
}
__global__ __launch_bounds__(256) void slot_unpack_kernel(const SlotSegment* __restrict__ segs, int n_seg, int slot, const int* __restrict__ step,
                                                          char* image, long image_bytes, long per_block) {
    slot_move<false>(segs, n_seg, slot, step, image, image_bytes, per_block);
}

int grid_for(long image_bytes, int cus, long* per_block) {
    const long tiles = (image_bytes + 4095) / 4096;
    long blocks = std::min<long>(tiles, (long)std::max(cus, 1) * 8);         // 8 workgroups of 4 waves per CU: 32 waves hide the latency of one 16-byte access each
    blocks = std::max<long>(blocks, 1);
    *per_block = ((tiles + blocks - 1) / blocks) * 4096;
    return (int)((image_bytes + *per_block - 1) / *per_block);
}

template <bool PACK>
int launch_move(const SlotSegment* d_segs, int n_seg, int slot, const int* d_step, char* image, long image_bytes, int cus, hipStream_t st) {
    SVA_CHECK(d_segs && n_seg >= 1 && slot >= 0 && image && image_bytes >= 16 && image_bytes % 16 == 0, "slot pack: bad arguments");
    SVA_CHECK((reinterpret_cast<uintptr_t>(image) & 15) == 0, "slot pack: the image must be 16-byte aligned");
    long per_block = 0;
    const int grid = grid_for(image_bytes, cus, &per_block);
    if (PACK) hipLaunchKernelGGL(slot_pack_kernel, dim3(grid), dim3(256), 0, st, d_segs, n_seg, slot, d_step, image, image_bytes, per_block);
    else hipLaunchKernelGGL(slot_unpack_kernel, dim3(grid), dim3(256), 0, st, d_segs, n_seg, slot, d_step, image, image_bytes, per_block);
    SVA_HIP(hipGetLastError());
    return 0;
}

}  // namespace

int launch_slot_pack(const SlotSegment* d_segs, int n_seg, int slot, const int* d_step, void* image, long image_bytes, int cus, hipStream_t st) {
    return launch_move<true>(d_segs, n_seg, slot, d_step, static_cast<char*>(image), image_bytes, cus, st);
}
int launch_slot_unpack(const SlotSegment* d_segs, int n_seg, int slot, const int* d_step, const void* image, long image_bytes, int cus, hipStream_t st) {
    return launch_move<false>(d_segs, n_seg, slot, d_step, const_cast<char*>(static_cast<const char*>(image)), image_bytes, cus, st);
}

int check_slot_segments(const SlotSegments& L) {
    long off = 0;
    SVA_CHECK(!L.seg.empty(), "slot segments: empty table");
    for (const SlotSegment& s : L.seg) {
        SVA_CHECK(s.elem == 2 || s.elem == 4, "slot segments: elements are 2 or 4 bytes");
        SVA_CHECK(s.rows >= 0 && s.row_bytes >= s.elem && s.row_bytes % s.elem == 0, "slot segments: a row is a whole number of elements");
        SVA_CHECK(s.row_stride >= s.row_bytes && s.row_stride % s.elem == 0 && s.slot_stride >= 0 && s.slot_stride % s.elem == 0, "slot segments: strides");
        SVA_CHECK((reinterpret_cast<uintptr_t>(s.base) % s.elem) == 0, "slot segments: base not aligned to its element");
        SVA_CHECK(s.kind >= kSegPlain && s.kind <= kSegBlockedPlane, "slot segments: unknown kind");
        SVA_CHECK(s.kind != kSegRing || (s.rows == 1 && s.ring_step >= 0), "slot segments: a ring is one row");
        SVA_CHECK(s.img_off == off && off % 16 == 0, "slot segments: image offsets must be the running sum of the padded lengths");
        off += seg_padded(s);
    }
    SVA_CHECK(off == L.image_bytes && off >= 16, "slot segments: image length");
    return 0;
}

}  // namespace sva
