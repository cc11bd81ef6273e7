// Which instantiation a launch of the dense pipeline, an any-hit walk or a short queue takes, as pure functions of the facts the host knows.
// Decisions only: no hip* call, no rt_ctx.  The kernel tables of rt_ctx.h are indexed by what these functions return, rt_create fills the
// resident grids over the same tables, and the device-free rt_launch_form (include/rt_amd.h) hands the same answers to tests/test_forms_cpu.py,
// which holds them to a restatement of the ladders they replaced (tests/forms_ref.py).
// A new form is a bit (or an enumerator) here, an entry in the family's table in rt_ctx.h and a case in tests/forms_ref.py.
#pragma once
#include <cstddef>

// A dense batch in raw facts, as run_rounds_stream learns them
struct DenseBatch {
	bool table;        // the primary-hit table is current (primary_table_for *use)
	bool bounceTable;  // ... and the bounce table (*bounce)
	int chainLevels;   // the chain levels the batch may read, 1 (the bounce table alone) .. 4 (*chain)
	bool bounceKnob;   // knobs.bounceTable != 0
	int round0Entries; // knobs.round0Entries
	bool sampler;      // Qt.on
	bool fisheye;      // C.fisheye
	int rounds;
	// the sampler's shade keeps emit_ray_s: the same bits either way
	bool bounce() const { return bounceTable && bounceKnob && !sampler; }
	// rounds 1 .. chainDepth - 1 read the chain tables (k_shade_s CHAIN), round 0 hands them their keys; a batch whose round 1 is its last has no use for them
	int chainDepth() const { return bounce() && rounds > 2 ? chainLevels : 1; }
	// round 0 straight from the table (k_generate_c, k_shade_s / k_light_s TABLE0): no round-0 entry is written or read.  The pinhole ray is
	// what the kernels rebuild from the pixel, and the sampler's shade keeps its entries; RT_ROUND0_ENTRIES=1 keeps them for everybody.
	bool direct() const { return table && !sampler && !fisheye && round0Entries != 1; }
};

// k_shade_s<QL, BOUNCE, TABLE0, CHAIN>: the form is the index of the instantiation in the family's table
enum { SHADE_QL = 1, SHADE_BOUNCE = 2, SHADE_TABLE0 = 4, SHADE_CHAIN = 8, SHADE_FORMS = 16 };
static inline int shade_form(const DenseBatch& b, int round)
{
	const bool last = round + 1 == b.rounds;
	if (b.sampler) return SHADE_QL;
	if (round == 0) return (b.direct() ? SHADE_TABLE0 : 0) | (b.chainDepth() > 1 ? SHADE_CHAIN : 0) | (b.bounce() && !last ? SHADE_BOUNCE : 0);
	return round < b.chainDepth() && !last ? SHADE_CHAIN : 0;
}
// what a shade launch of a form is handed: where its BounceTable and PrimaryTable arguments come from, and fresh / the bounce mask
enum { BT_EMPTY = 0, BT_BOUNCE = 1, BT_CHAIN = 2 }; // BT_CHAIN: level round + 1, chain[round - 1]
static inline int shade_bt(int form) { return form & SHADE_BOUNCE ? BT_BOUNCE : form & SHADE_CHAIN ? BT_CHAIN : BT_EMPTY; }
static inline bool shade_masked(int form) { return (form & (SHADE_BOUNCE | SHADE_CHAIN)) != 0; }
static inline bool shade_tab(int form) { return (form & SHADE_TABLE0) != 0; }

// k_light_s<TABLE0> over the shadow records of round 'round'
enum { LIGHT_FORMS = 2 };
static inline int light_form(const DenseBatch& b, int round) { return b.direct() && round == 0 ? 1 : 0; }

// k_generate_c / k_generate_t / k_generate_s
enum { GENERATE_C = 0, GENERATE_T = 1, GENERATE_S = 2 };
static inline int generate_form(const DenseBatch& b) { return b.direct() ? GENERATE_C : b.table ? GENERATE_T : GENERATE_S; }

// Scene::IsOccluded for a queue of rays.  Counting launches walk like the reference; timed launches take the 8-wide or the 4-wide walk when
// the scene has such nodes, followed by the binary walk over the (normally empty) list of rays the wide walk handed back because they are
// not clean (WALK_LISTED: never chosen, always the second launch behind a wide walk).
enum { WALK_BINARY = 0, WALK_COUNTING = 1, WALK_WIDE4 = 2, WALK_LISTED = 3, WALK_WIDE8 = 4, WALK_FORMS = 5 };
static inline int any_hit_walk(bool counting, bool wide, bool wide8) { return counting ? WALK_COUNTING : wide8 ? WALK_WIDE8 : wide ? WALK_WIDE4 : WALK_BINARY; }
static inline bool walk_is_wide(int walk) { return walk == WALK_WIDE4 || walk == WALK_WIDE8; }

// a short queue does not need the whole resident grid (chunk: the queue entries a wave reserves at a time, RT_CHUNK)
static inline int short_grid(size_t n, int resident, int chunk)
{
	const size_t g = (n + chunk - 1) / chunk / 4 + 1;
	return g > (size_t)resident ? resident : (int)g;
}
