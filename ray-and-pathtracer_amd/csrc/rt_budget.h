// Budgeted adaptive passes: every active pixel gets its OWN number of samples, and a pass runs them all as one batch.
// rt_select_budget makes rt_select_active's list (same predicate, same storage, same order) and, per list entry, a budget b from the
// pixel's variance (include/rt_amd.h rt_select_budget, restated in tests/budget_ref.py: f32, IEEE division, no contraction), the pixel's
// count at selection time (its first frame) and the exclusive prefix sum of the budgets (where its samples start in the pool).  The
// pool is entry-major: the b samples of an entry are adjacent, in frame order, so a wave's camera rays leave neighbouring pixels and
// k_accumulate_budget reads a contiguous run.  Sample sid of the pool is the (pixel, frame) pair its 8-byte record names -- the one
// load sample_pixel_frame (rt_kernels.h) makes for a budgeted batch.
// The house pattern of rt_adaptive.h, no block waits on another:
//   k_budget_count    a block of RT_SELECT_BLOCK lanes owns that many consecutive pixels of the row set (rt_adaptive.h RowMap): its active
//                     pixels and the sum of their budgets
//   k_budget_scan     ONE block: exclusive scans of both block totals in place; the grand totals (pixels: int, budgets: 64 bit)
//   k_budget_scatter  predicate and budget again; list / budget / first frame / offset per entry, then the wave expands its entries'
//                     records TOGETHER: lanes stride over the wave's range of the pool and find their entry in the wave's prefix sums
//                     (one lane per entry would serialise the wave behind its noisiest pixel: up to 1024 records)
// The count runs once per cap tried (the fit rule: cap = pass_cap >> k), the scatter once, after the total has been read back and fits.
// Count and scatter are written once, as budget_count_body / budget_scatter_body over a lane source; the kernels name the source
// (here the row set, in rt_dilate.h the listed mask of the dilated selection).
#pragma once
#include "rt_adaptive.h"

namespace rtd {

struct BudgetPlan {
	uint* budget;   // [entry] samples of this pass
	uint* first;    // [entry] the pixel's count at selection time: sample k of the entry is frame frame_base + first + k
	uint* offset;   // [entry] exclusive prefix sum of the budgets: the entry's first sample in the pool
	uint2* records; // [sample] { pixel, first + k }
};

// include/rt_amd.h rt_select_budget, line by line; 0: the pixel is not active.  The predicate is rt_adaptive.h's own (pixel_noisy on
// pixel_moments), and the budget is made from the same n, v and d.
__device__ __forceinline__ uint pixel_budget(uint count, float sumY, float sumYY, const AdaptiveArgs& A, int cap)
{
	int b;
	if (count < (uint)A.minSamples) b = A.minSamples - (int)count;
	else {
		const PixelMoments M = pixel_moments(count, sumY, sumYY, A);
		if (!pixel_noisy(count, sumY, sumYY, A, M)) return 0;
		const float g = A.threshold * M.d;
		const float t = M.v / (g * g);
		const float need = t - M.n;
		b = need >= (float)cap ? cap : (need >= 1.0f ? (int)ceilf(need) : 1);
	}
	b = min(b, cap);
	b = min(b, A.maxSamples - (int)count);
	return (uint)b;
}

// What decides a lane of the count and the scatter below: a source has one method, lane(i) -> the pixel lane i stands for, its count
// at selection time and its budget (0: not listed; pixel and count are then not used).  The row-set source walks rt_adaptive.h's RowMap;
// rt_dilate.h has the one that walks the listed mask.
struct BudgetLane { uint pixel, count, budget; };
struct RowSetSource {
	PixelStats St;
	AdaptiveArgs A;
	int cap;
	RowMap M;
	__device__ __forceinline__ BudgetLane lane(int i) const
	{
		if (i >= M.nPixels) return BudgetLane{ 0u, 0u, 0u };
		const int p = row_map_pixel(M, i);
		const uint count = St.count[p];
		return BudgetLane{ (uint)p, count, pixel_budget(count, St.sumY[p], St.sumYY[p], A, cap) };
	}
};

// a block of RT_SELECT_BLOCK lanes: its listed pixels and the sum of their budgets
template <class Source> __device__ __forceinline__ void budget_count_body(const Source& S, uint* blockPixels, uint* blockBudget)
{
	__shared__ uint wavePixels[RT_SELECT_BLOCK / 64], waveBudget[RT_SELECT_BLOCK / 64];
	const uint b = S.lane(blockIdx.x * RT_SELECT_BLOCK + threadIdx.x).budget;
	const uint lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const bits64 mask = __ballot(b != 0);
	const uint incl = wave_inclusive(b, lane);
	if (lane == 63) wavePixels[wave] = (uint)__popcll(mask), waveBudget[wave] = incl;
	__syncthreads();
	if (threadIdx.x == 0) {
		uint pixels = 0, budget = 0; // a block's budgets: at most RT_SELECT_BLOCK * 1024
		for (int w = 0; w < RT_SELECT_BLOCK / 64; w++) pixels += wavePixels[w], budget += waveBudget[w];
		blockPixels[blockIdx.x] = pixels, blockBudget[blockIdx.x] = budget;
	}
}

__global__ void __launch_bounds__(RT_SELECT_BLOCK) k_budget_count(PixelStats St, AdaptiveArgs A, int cap, RowMap M, uint* blockPixels, uint* blockBudget)
{
	budget_count_body(RowSetSource{ St, A, cap, M }, blockPixels, blockBudget);
}

// one block: both arrays -> their exclusive prefix sums; *nActive and *nSamples the totals.  The budgets are summed in 64 bits (a 4K frame
// at 1024 samples per pixel is past 2^32); the prefix sums are stored as 32-bit words, which is what they are whenever the total fits a
// pass -- the only case in which the scatter runs and reads them.
__global__ void __launch_bounds__(RT_SELECT_SCAN_BLOCK) k_budget_scan(uint* blockPixels, uint* blockBudget, int nBlocks, int* nActive, unsigned long long* nSamples)
{
	__shared__ uint wavePixels[RT_SELECT_SCAN_BLOCK / 64];
	__shared__ unsigned long long waveBudget[RT_SELECT_SCAN_BLOCK / 64];
	const int per = (nBlocks + RT_SELECT_SCAN_BLOCK - 1) / RT_SELECT_SCAN_BLOCK;
	const int first = min((int)threadIdx.x * per, nBlocks), last = min(first + per, nBlocks);
	uint minePixels = 0;
	unsigned long long mineBudget = 0;
	for (int i = first; i < last; i++) minePixels += blockPixels[i], mineBudget += blockBudget[i];
	const uint lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	uint inclPixels = minePixels;
	unsigned long long inclBudget = mineBudget;
	for (int o = 1; o < 64; o <<= 1) {
		const uint tp = __shfl_up(inclPixels, o);
		const uint lo = __shfl_up((uint)inclBudget, o), hi = __shfl_up((uint)(inclBudget >> 32), o);
		if ((int)lane >= o) inclPixels += tp, inclBudget += ((unsigned long long)hi << 32) | lo;
	}
	if (lane == 63) wavePixels[wave] = inclPixels, waveBudget[wave] = inclBudget;
	__syncthreads();
	uint basePixels = 0, totalPixels = 0;
	unsigned long long baseBudget = 0, totalBudget = 0;
	for (int w = 0; w < RT_SELECT_SCAN_BLOCK / 64; w++) {
		if (w < (int)wave) basePixels += wavePixels[w], baseBudget += waveBudget[w];
		totalPixels += wavePixels[w], totalBudget += waveBudget[w];
	}
	uint atPixels = basePixels + inclPixels - minePixels;
	unsigned long long atBudget = baseBudget + inclBudget - mineBudget;
	for (int i = first; i < last; i++) {
		const uint tp = blockPixels[i], tb = blockBudget[i];
		blockPixels[i] = atPixels, blockBudget[i] = (uint)atBudget;
		atPixels += tp, atBudget += tb;
	}
	if (threadIdx.x == 0) *nActive = (int)totalPixels, *nSamples = totalBudget;
}

// Runs only after the host has seen that the total of the budgets fits the pool (nSamples records).  Entries: at < the total of the
// listed pixels <= the lanes of the launch; records: below the total of the budgets -- the count and this body evaluate one source on the
// same statistics.
template <class Source> __device__ __forceinline__ void budget_scatter_body(const Source& S, const uint* pixelBase, const uint* budgetBase, uint* list, BudgetPlan B)
{
	__shared__ uint wavePixels[RT_SELECT_BLOCK / 64], waveBudget[RT_SELECT_BLOCK / 64];
	const BudgetLane L = S.lane(blockIdx.x * RT_SELECT_BLOCK + threadIdx.x); // L.pixel: what the list and the records name
	const uint b = L.budget;
	const uint lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const bits64 mask = __ballot(b != 0);
	const uint incl = wave_inclusive(b, lane); // non-decreasing over the lanes: an unlisted lane adds 0
	if (lane == 63) wavePixels[wave] = (uint)__popcll(mask), waveBudget[wave] = incl;
	__syncthreads();
	uint at = pixelBase[blockIdx.x], waveOffset = budgetBase[blockIdx.x];
	for (uint w = 0; w < wave; w++) at += wavePixels[w], waveOffset += waveBudget[w];
	if (b != 0) {
		at += lanes_below(mask);
		list[at] = L.pixel, B.budget[at] = b, B.first[at] = L.count, B.offset[at] = waveOffset + incl - b;
	}
	// the wave's records: record j of the wave belongs to the first lane whose inclusive sum is past j
	const uint waveSamples = waveBudget[wave];
	for (uint j0 = 0; j0 < waveSamples; j0 += 64) { // (wave-uniform trip count: every lane takes part in the shuffles)
		const uint j = j0 + lane;
		uint owner = 0;
		for (uint step = 32; step; step >>= 1) {
			const uint probe = __shfl(incl, (int)(owner + step - 1));
			if (probe <= j) owner += step;
		}
		const int src = (int)min(owner, 63u); // (j >= waveSamples: no owner, nothing written)
		const uint ownerPixel = __shfl(L.pixel, src), ownerCount = __shfl(L.count, src), ownerStart = __shfl(incl - b, src);
		if (j < waveSamples) B.records[waveOffset + j] = make_uint2(ownerPixel, ownerCount + (j - ownerStart));
	}
}

__global__ void __launch_bounds__(RT_SELECT_BLOCK) k_budget_scatter(PixelStats St, AdaptiveArgs A, int cap, RowMap M, const uint* pixelBase, const uint* budgetBase, uint* list, BudgetPlan B)
{
	budget_scatter_body(RowSetSource{ St, A, cap, M }, pixelBase, budgetBase, list, B);
}

// k_accumulate<true> (rt_kernels.h) with lane = list entry: the entry's b samples, adjacent in the pool, in frame order
__global__ void k_accumulate_budget(RenderParams R, const uint* list, BudgetPlan B, int nEntries, PixelStats St)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= nEntries) return;
	const uint pixel = list[i], b = B.budget[i], off = B.offset[i];
	float4 a = R.accum[pixel];
	float sy = St.sumY[pixel], syy = St.sumYY[pixel];
	for (uint k = 0; k < b; k++) add_sample<true>(R.samples[off + k], a, sy, syy);
	R.accum[pixel] = a;
	St.count[pixel] += b, St.sumY[pixel] = sy, St.sumYY[pixel] = syy;
}

} // namespace rtd
