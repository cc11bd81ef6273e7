// Dilated adaptive selection: a pixel is listed when it is active by rt_select_active's predicate ("raw"), or when it may still take a
// sample ("eligible": below max_samples, finite sums) and a raw-active pixel lies within 'radius' pixels of it on both axes, the window
// clipped to the frame (include/rt_amd.h rt_select_active_dilated, restated in tests/dilate_ref.py).  A pixel that missed a rare bright
// path looks converged from its own statistics; its neighbours that saw one keep it sampling.
// No kernel reads a neighbour's statistics: the predicate is evaluated once per pixel and kept as ONE BIT, and everything after works on
// bitmasks over the linear pixel index p = y * width + x (word p >> 6, bit p & 63; a frame's masks fit the L2: width * height / 8 bytes
// each).  Whole frame only: lane i of a launch is pixel i, blocks of RT_SELECT_BLOCK lanes, so a wave's __ballot IS word i >> 6 of a mask and
// lane 0 of the wave stores it; a lane past the frame votes 0, which leaves the high bits of the last word clear.
//   k_dilate_mask     the 12 B of statistics, once: the raw and the eligible mask
//   k_dilate_rows     horizontal: bit p of 'rows' = OR of raw over the row window [max(p - r, row start), min(p + r, row end)] -- a run
//                     of at most 2 r + 1 <= 33 bits of the linear index, in at most two words; clipping the run to the pixel's own row is
//                     all the row clip there is, whatever the width is to 64 (several rows in a word, a row across words)
//   k_dilate_cols     vertical: listed = raw || (eligible && OR of single bits of 'rows' at p + dy * width, rows y + dy inside the frame);
//                     stores the listed mask and the block's total -- k_select_count's part in the compaction, by its block_total_of
//   k_select_scan     rt_adaptive.h's own, unchanged
//   k_dilate_scatter  k_select_scatter on the listed mask: a bit per lane instead of the predicate, into the same scatter_listed
// The vertical OR costs up to 33 bit reads, so it runs once and its result is kept as a fourth mask: the scatter, and the budget form's
// count (once per cap tried) and scatter, read one word per wave instead of walking the column again.
// The budget form (rt_select_budget_dilated) makes rt_budget.h's plan over the listed mask: a raw-active pixel gets pixel_budget, a pixel
// listed by dilation alone gets 1; only listed pixels' statistics are read (their own).  Its count and scatter are rt_budget.h's bodies
// over DilatedSource; the scan is k_budget_scan, unchanged.
#pragma once
#include "rt_budget.h"

namespace rtd {

struct DilateMasks {
	bits64* raw;      // rt_select_active's predicate
	bits64* eligible; // count < max_samples && isfinite(sum_y) && isfinite(sum_yy)
	bits64* rows;     // raw, dilated along the rows
	bits64* listed;   // the result
};

__device__ __forceinline__ bool mask_bit(const bits64* mask, int p) { return (mask[p >> 6] >> (p & 63)) & 1ull; }

__global__ void __launch_bounds__(RT_SELECT_BLOCK) k_dilate_mask(PixelStats St, AdaptiveArgs A, int nPixels, bits64* raw, bits64* eligible)
{
	const int i = blockIdx.x * RT_SELECT_BLOCK + threadIdx.x;
	bool on = false, may = false;
	if (i < nPixels) {
		const uint count = St.count[i];
		const float sumY = St.sumY[i], sumYY = St.sumYY[i];
		on = pixel_active(count, sumY, sumYY, A);
		may = count < (uint)A.maxSamples && isfinite(sumY) && isfinite(sumYY);
	}
	const bits64 onBits = __ballot(on), mayBits = __ballot(may);
	// lane 0 of a wave is pixel 64 * word: inside the frame exactly when the word exists
	if ((threadIdx.x & 63) == 0 && i < nPixels) raw[i >> 6] = onBits, eligible[i >> 6] = mayBits;
}

__global__ void __launch_bounds__(RT_SELECT_BLOCK) k_dilate_rows(const bits64* raw, int nPixels, int width, int radius, bits64* rows)
{
	const int i = blockIdx.x * RT_SELECT_BLOCK + threadIdx.x;
	bool on = false;
	if (i < nPixels) {
		const int rowStart = (i / width) * width;
		const int lo = max(i - radius, rowStart), hi = min(i + radius, rowStart + width - 1); // hi < nPixels: the row ends inside the frame
		const int wordLo = lo >> 6, wordHi = hi >> 6;                                        // hi - lo <= 32: the same word or the next
		const bits64 low = raw[wordLo] >> (lo & 63);                                         // bit 0: pixel lo
		if (wordLo == wordHi) on = (low & ((1ull << (hi - lo + 1)) - 1)) != 0;
		else on = low != 0 || (raw[wordHi] & ((2ull << (hi & 63)) - 1)) != 0;                // bits 0 .. hi & 63 of the next word
	}
	const bits64 bits = __ballot(on);
	if ((threadIdx.x & 63) == 0 && i < nPixels) rows[i >> 6] = bits;
}

__global__ void __launch_bounds__(RT_SELECT_BLOCK) k_dilate_cols(DilateMasks D, int nPixels, int width, int height, int radius, uint* blockTotal)
{
	const int i = blockIdx.x * RT_SELECT_BLOCK + threadIdx.x;
	bool on = false;
	if (i < nPixels) {
		on = mask_bit(D.raw, i);
		if (!on && mask_bit(D.eligible, i)) {
			const int y = i / width;
			const int first = i - min(radius, y) * width, last = i + min(radius, height - 1 - y) * width; // rows y - r .. y + r inside the frame
			for (int q = first; q <= last && !on; q += width) on = mask_bit(D.rows, q);
		}
	}
	const bits64 bits = __ballot(on);
	if ((threadIdx.x & 63) == 0 && i < nPixels) D.listed[i >> 6] = bits;
	block_total_of(bits, blockTotal);
}

// k_dilate_cols counted the bits of this mask
__global__ void __launch_bounds__(RT_SELECT_BLOCK) k_dilate_scatter(const bits64* listed, int nPixels, const uint* blockBase, uint* list)
{
	const int i = blockIdx.x * RT_SELECT_BLOCK + threadIdx.x;
	scatter_listed(i < nPixels ? listed[i >> 6] : 0ull, (uint)i, blockBase, list); // the wave's word (a wave past the frame has none)
}

// rt_budget.h's source over the listed mask, lane i = pixel i: rt_select_budget's budget on a raw-active pixel, 1 on a pixel listed by
// dilation alone, 0 unlisted.  Only listed pixels' statistics are read.
struct DilatedSource {
	DilateMasks D;
	PixelStats St;
	AdaptiveArgs A;
	int cap, nPixels;
	__device__ __forceinline__ BudgetLane lane(int i) const
	{
		if (i >= nPixels || !mask_bit(D.listed, i)) return BudgetLane{ (uint)i, 0u, 0u };
		const uint count = St.count[i];
		if (!mask_bit(D.raw, i)) return BudgetLane{ (uint)i, count, 1u };
		return BudgetLane{ (uint)i, count, pixel_budget(count, St.sumY[i], St.sumYY[i], A, cap) }; // >= 1: the raw mask is pixel_active of these statistics
	}
};

__global__ void __launch_bounds__(RT_SELECT_BLOCK) k_dilate_budget_count(DilateMasks D, PixelStats St, AdaptiveArgs A, int cap, int nPixels, uint* blockPixels, uint* blockBudget)
{
	budget_count_body(DilatedSource{ D, St, A, cap, nPixels }, blockPixels, blockBudget);
}

__global__ void __launch_bounds__(RT_SELECT_BLOCK) k_dilate_budget_scatter(DilateMasks D, PixelStats St, AdaptiveArgs A, int cap, int nPixels, const uint* pixelBase, const uint* budgetBase, uint* list, BudgetPlan B)
{
	budget_scatter_body(DilatedSource{ D, St, A, cap, nPixels }, pixelBase, budgetBase, list, B);
}

} // namespace rtd
