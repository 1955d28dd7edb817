// Launchers of snapshot/slot_pack.hip: one slot's segments (slot_state.h) <-> one contiguous device image.
#pragma once
#include "slot_state.h"

namespace sva {

// Every segment of slot `slot` of the table `d_segs` (device memory, n_seg entries, img_off ascending) into `image` (16-byte aligned,
// image_bytes = the sum of the padded segment lengths): payload bytes copied, padding written as zeros.  A ring segment is stored
// un-rotated: its origin is read from *d_step on the device.  cus: compute units of the stream (sizes the grid).  One launch on st.
int launch_slot_pack(const SlotSegment* d_segs, int n_seg, int slot, const int* d_step, void* image, long image_bytes, int cus, hipStream_t st);
// The reverse: payload bytes of the image into the slot's rows (a ring segment at the rotation *d_step gives); nothing else is written.
int launch_slot_unpack(const SlotSegment* d_segs, int n_seg, int slot, const int* d_step, const void* image, long image_bytes, int cus, hipStream_t st);
// host-side check of a table before it is uploaded: element sizes, multiples, ascending 16-byte image offsets, ring shape
int check_slot_segments(const SlotSegments& L);

}  // namespace sva
