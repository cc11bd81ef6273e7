// Several contexts, adaptive passes (rt_gather_active): after a pass only the listed pixels of a context have changed, so only they are
// pushed to the context that holds the gathered frame -- 28 B per listed pixel instead of 28 B per pixel of the shard's rows.
//   k_push_active   one lane per list entry: the entry's accumulator value (one 16-byte load) and its count, sum_y and sum_yy from the
//                   source's arrays, stored to the same pixel of the destination's arrays.  The destination's pointers arrive by value:
//                   memory of the same device, or of a peer the source's device has mapped (rt_api_gather.inc enables the access as
//                   rt_gather_rows does).  Plain vector stores: a pixel is on the list once, and the destination's own queued work does
//                   not write the listed pixels (the call's contract), so nothing needs an atomic.
// The list ascends, so a run of listed neighbours is a run of neighbouring lanes: their loads and stores coalesce (16 B and 4 B per lane);
// an isolated entry costs a 64-byte segment per array on either side.
#pragma once
#include "rt_kernels.h" // PixelStats

namespace rtd {

#define RT_PUSH_BLOCK 256

__global__ void __launch_bounds__(RT_PUSH_BLOCK) k_push_active(const uint* list, int nEntries, const float4* accum, PixelStats St, float4* dstAccum, PixelStats dstSt)
{
	const int i = blockIdx.x * RT_PUSH_BLOCK + threadIdx.x;
	if (i >= nEntries) return;
	const uint p = list[i]; // < width * height of both contexts: rt_set_active_pixels checks it, the selections make nothing else
	const float4 a = accum[p];
	const uint count = St.count[p];
	const float sy = St.sumY[p], syy = St.sumYY[p];
	dstAccum[p] = a;
	dstSt.count[p] = count, dstSt.sumY[p] = sy, dstSt.sumYY[p] = syy;
}

} // namespace rtd
