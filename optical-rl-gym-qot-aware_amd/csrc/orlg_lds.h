// orlg_lds.h -- the LDS of a CU (gfx950): what the host sizes the workgroups of every step kernel against.  On its own so that no
// kernel object depends on it.
#pragma once
#define ORLG_LDS_BYTES (160 * 1024)
