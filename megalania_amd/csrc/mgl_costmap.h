/*
 * mgl_costmap.h -- what the two cost maps share: the serial walk of mgl_costmap.hip, which costs any
 * slab under any layout, and the parallel pass of mgl_costmap_live.hip, which reads the current slab's cost off the event
 * chains.  The mark word, the classes, the sums both hand to the host.
 */
#pragma once
#include "mgl_device.h"

#define MGL_CM_CLASSES 6u      /* MGL_CC_*: kind, literal, length, rep length, distance, direct */
#define MGL_CM_COST_BITS 20u   /* a mark: cost | len << 20 */
/* at most MGL_MAX_EVENTS modelled bits of at most 22 528 (the table's largest entry) and 26 direct bits of 2 048 */
static_assert(MGL_MAX_EVENTS * 22528u + 26u * 2048u < (1u << MGL_CM_COST_BITS), "a packet's cost must fit its mark");
static_assert(MGL_MAX_MATCH < (1u << (32u - MGL_CM_COST_BITS)), "a packet's length must fit its mark");

struct CostMapSums {
	uint64_t total, packets;
	uint64_t class_cost[MGL_CM_CLASSES], class_bits[MGL_CM_CLASSES];
	uint64_t type_cost[4], type_packets[4], type_bytes[4];
	uint32_t end_pos, pad; /* where the walk stopped: n for a slab the walk of mgl_cost_slab accepts */
};

/* the coder a context index belongs to, as an MGL_CC_* number (never MGL_CC_DIRECT: direct bits have no context) */
__device__ __forceinline__ uint32_t costmap_class(uint32_t ctx)
{
	return ctx < MGL_OFF_LEN ? 0u : ctx < MGL_OFF_REP_LEN ? 2u : ctx < MGL_OFF_DIST ? 3u : ctx < MGL_OFF_LIT ? 4u : 1u;
}

/* the direct bits of a packet, from its type and distance alone: mgl_plan_packet's rule (a MATCH whose distance slot is 14
 * or more codes the bits between the slot's two and the align tree's four directly) */
__device__ __forceinline__ uint32_t costmap_ndirect(uint32_t type, uint32_t dist)
{
	if (type != MGL_MATCH || dist < 4u) return 0u;
	const uint32_t nlow = mgl_msb32(dist) - 2u;
	return nlow * 2u + (dist >> nlow) < 14u ? 0u : nlow - 4u;
}
