// Adaptive sampling: the per-pixel statistics' consumers.  k_accumulate<true> (rt_kernels.h) keeps count / sum_y / sum_yy per pixel;
// here the list of pixels that still need samples is made from them (rt_select_active), in ascending pixel order, and the frame is
// resolved with every pixel's own count (rt_resolve_adaptive).  The predicate is defined in include/rt_amd.h (rt_select_active) and
// restated in numpy in tests/adaptive_ref.py; the two follow each other operation by operation (f32, IEEE division and square root,
// no contraction: the library is built with -ffp-contract=off).
// The compaction is three launches on the context's stream -- a block's count, one block's scan of the block counts, the scatter --
// so that no block ever waits for another one (the house pattern of compact_body / k_assign: counts first, positions from a scan).
//   k_select_count    a block of RT_SELECT_BLOCK lanes owns RT_SELECT_BLOCK consecutive pixels of the row set: ballot per wave, the block's total
//   k_select_scan     ONE block: exclusive scan of the block totals in place, the grand total to *nActive
//   k_select_scatter  the predicate again (12 B per pixel: cheaper than keeping a flag array), rank inside the wave by mbcnt,
//                     list[block base + waves before + rank] = pixel
// The launches walk a ROW SET (RowMap: rows rowFirst + k * rowStride, k < rowCount -- the share of the frame a context renders when the
// rows are interleaved over several contexts, rt_select_active_rows): lane i owns the i-th pixel of the set in ascending pixel order, so
// a shard reads only its own rows' statistics and its list ascends.  The whole frame is the set (0, 1, height), where i is the pixel.
// What count and scatter do with a wave's ballot (block_total_of, scatter_listed) is shared with the dilated selection of rt_dilate.h,
// whose lanes are decided by a bit of a mask instead of the predicate.
#pragma once
#include "rt_kernels.h" // PixelStats, resolve_pixel

namespace rtd {

#define RT_SELECT_BLOCK 256
#define RT_SELECT_SCAN_BLOCK 1024

struct AdaptiveArgs {
	int minSamples, maxSamples;
	float threshold, floor;
};

struct RowMap {
	int rowFirst, rowStride, width;
	int nPixels; // rowCount * width
};
// lane i < nPixels -> its pixel; strictly ascending in i (rowStride >= 1).  Consecutive rows need no division.
__device__ __forceinline__ int row_map_pixel(const RowMap& M, int i)
{
	if (M.rowStride == 1) return M.rowFirst * M.width + i;
	const int k = i / M.width;
	return (M.rowFirst + k * M.rowStride) * M.width + (i - k * M.width);
}

// include/rt_amd.h rt_select_active, line by line: n, m, v (after its clamp) and d of a pixel with samples, shared with the budget
// of rt_budget.h, so that the list and the plan cannot come apart
struct PixelMoments { float n, m, v, d; };
__device__ __forceinline__ PixelMoments pixel_moments(uint count, float sumY, float sumYY, const AdaptiveArgs& A)
{
	PixelMoments M;
	M.n = (float)count;
	M.m = sumY / M.n;
	M.v = (sumYY - sumY * M.m) / (M.n - 1);
	M.v = M.v > 0 ? M.v : 0;
	M.d = M.m > A.floor ? M.m : A.floor;
	return M;
}
// a pixel at or above min_samples: is it still noisy?
__device__ __forceinline__ bool pixel_noisy(uint count, float sumY, float sumYY, const AdaptiveArgs& A, const PixelMoments& M)
{
	if (count >= (uint)A.maxSamples || !isfinite(sumY) || !isfinite(sumYY)) return false;
	const float e = sqrtf(M.v / M.n);
	return e / M.d > A.threshold;
}
__device__ __forceinline__ bool pixel_active(uint count, float sumY, float sumYY, const AdaptiveArgs& A)
{
	if (count < (uint)A.minSamples) return true;
	return pixel_noisy(count, sumY, sumYY, A, pixel_moments(count, sumY, sumYY, A));
}

typedef unsigned long long bits64; // a wave's ballot; a word of the bitmasks of rt_dilate.h

// lanes of this wave below the caller that are set in 'mask'
__device__ __forceinline__ uint lanes_below(bits64 mask)
{
	return __builtin_amdgcn_mbcnt_hi((uint)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint)mask, 0u));
}

// inclusive prefix sum over the wave
__device__ __forceinline__ uint wave_inclusive(uint v, uint lane)
{
	for (int o = 1; o < 64; o <<= 1) { const uint t = __shfl_up(v, o); if ((int)lane >= o) v += t; }
	return v;
}

// The two tails of the list form, shared by the row-set kernels below and the dilated ones of rt_dilate.h: 'mask' is the wave's ballot of
// its listed lanes (or the word of the listed mask that holds the same bits).
// count: blockTotal[this block] = the listed lanes of its waves
__device__ __forceinline__ void block_total_of(bits64 mask, uint* blockTotal)
{
	__shared__ uint waveTotal[RT_SELECT_BLOCK / 64];
	if ((threadIdx.x & 63) == 0) waveTotal[threadIdx.x >> 6] = (uint)__popcll(mask);
	__syncthreads();
	if (threadIdx.x == 0) {
		uint sum = 0;
		for (int w = 0; w < RT_SELECT_BLOCK / 64; w++) sum += waveTotal[w];
		blockTotal[blockIdx.x] = sum;
	}
}
// scatter: list[block base + waves before + rank inside the wave] = pixel, for the lanes whose bit is set.  at < the grand total <= the
// lanes of the launch: the count pass made the totals from the same bits.
__device__ __forceinline__ void scatter_listed(bits64 mask, uint pixel, const uint* blockBase, uint* list)
{
	__shared__ uint waveTotal[RT_SELECT_BLOCK / 64];
	const uint wave = threadIdx.x >> 6;
	if ((threadIdx.x & 63) == 0) waveTotal[wave] = (uint)__popcll(mask);
	__syncthreads();
	if (!((mask >> (threadIdx.x & 63)) & 1ull)) return;
	uint at = blockBase[blockIdx.x] + lanes_below(mask);
	for (uint w = 0; w < wave; w++) at += waveTotal[w];
	list[at] = pixel;
}

__global__ void __launch_bounds__(RT_SELECT_BLOCK) k_select_count(PixelStats St, AdaptiveArgs A, RowMap M, uint* blockTotal)
{
	const int i = blockIdx.x * RT_SELECT_BLOCK + threadIdx.x;
	const int p = i < M.nPixels ? row_map_pixel(M, i) : 0;
	const bool on = i < M.nPixels && pixel_active(St.count[p], St.sumY[p], St.sumYY[p], A);
	block_total_of(__ballot(on), blockTotal);
}

// one block: blockTotal[0 .. nBlocks) -> its exclusive prefix sums, *nActive = the total.  A lane owns a run of consecutive entries.
__global__ void __launch_bounds__(RT_SELECT_SCAN_BLOCK) k_select_scan(uint* blockTotal, int nBlocks, int* nActive)
{
	__shared__ uint waveSum[RT_SELECT_SCAN_BLOCK / 64];
	const int per = (nBlocks + RT_SELECT_SCAN_BLOCK - 1) / RT_SELECT_SCAN_BLOCK;
	const int first = min((int)threadIdx.x * per, nBlocks), last = min(first + per, nBlocks);
	uint mine = 0;
	for (int i = first; i < last; i++) mine += blockTotal[i];
	const uint lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint incl = wave_inclusive(mine, lane);
	if (lane == 63) waveSum[wave] = incl;
	__syncthreads();
	uint base = 0, total = 0;
	for (int w = 0; w < RT_SELECT_SCAN_BLOCK / 64; w++) { if (w < (int)wave) base += waveSum[w]; total += waveSum[w]; }
	uint at = base + incl - mine;
	for (int i = first; i < last; i++) { const uint t = blockTotal[i]; blockTotal[i] = at; at += t; }
	if (threadIdx.x == 0) *nActive = (int)total;
}

// the predicate again: the three launches evaluate it on the same statistics
__global__ void __launch_bounds__(RT_SELECT_BLOCK) k_select_scatter(PixelStats St, AdaptiveArgs A, RowMap M, const uint* blockBase, uint* list)
{
	const int i = blockIdx.x * RT_SELECT_BLOCK + threadIdx.x;
	const int p = i < M.nPixels ? row_map_pixel(M, i) : 0;
	const bool on = i < M.nPixels && pixel_active(St.count[p], St.sumY[p], St.sumYY[p], A);
	scatter_listed(__ballot(on), (uint)p, blockBase, list);
}

// rt_resolve with the pixel's own sample count as the divisor; a pixel without samples is black
__global__ void k_resolve_adaptive(const float4* accum, const uint* count, int first, int n, uint* out)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint k = count[first + i];
	if (k == 0) { out[i] = 0; return; }
	out[i] = resolve_pixel(accum[first + i], (float)k);
}

} // namespace rtd
