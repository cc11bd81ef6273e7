// rt_set_materials on the device: the one thing a material table edit cannot do with a copy.  pack_prim (rt_layout.h) puts the type of a
// primitive's material into bits 4-5 of the record's kind word (RT_TYPE_SHIFT), where the traversal's flush reads it without a second fetch
// (rt_scene_dev.h); a material that changes its type therefore changes one word of every record that names it.  The yardstick is
// rt_set_instances's: afterwards the context holds, byte for byte, what rt_upload_scene would hold of the updated description.  What makes
// that possible without a host re-layout: the type bits are a function of the record's own material index and the table alone
// (pack_prim: (mats[mat].type & 3) << RT_TYPE_SHIFT for 0 <= mat < nMats, 0 otherwise), in every array of primitive records the context
// keeps -- prims[], the brute-force records, the originals rt_set_time deforms from -- and nothing else of a record depends on a material.
//
// Plain HIP C++ only.
#pragma once
#include "rt_kernels.h"

namespace rtd {

// A lane per 64-byte record.  A lane reads the record's last eight bytes {material, kind | last | type} as one dwordx2 -- a wave touches
// 64 records, every 128-byte line of them once -- and stores the kind word alone, and only where the type bits differ: a call that changes
// the type of a material few primitives name writes few lines.  The kind (bits 0-3), the last-of-leaf bit and every other word stay.
__global__ void __launch_bounds__(256) k_retype_prims(float4* recs, uint nRecs, const DMaterial* __restrict__ mats, int nMats)
{
	const uint i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= nRecs) return;
	int* const tail = (int*)(recs + 4 * (size_t)i) + 14; // words 14, 15 of the record: 8-byte aligned
	const int2 mk = *(const int2*)tail;
	const int mat = mk.x;
	int kl = mk.y & ~(3 << RT_TYPE_SHIFT);
	if (mat >= 0 && mat < nMats) kl |= (mats[mat].type & 3) << RT_TYPE_SHIFT;
	if (kl != mk.y) tail[1] = kl;
}

} // namespace rtd
