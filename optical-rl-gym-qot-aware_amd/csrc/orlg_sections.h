// orlg_sections.h -- section timing of the step kernels (debug builds): the SEC* macros and orlg_sections[].
//
// -DORLG_SECTIONS: wall cycles each wave spends in the sections of a step, summed over all waves into orlg_sections[]
// (tools/section_profile.py).  Not compiled into the product library.
#pragma once
#include "orlg_wave.h"

// section ids 0 .. ORLG_NSEC - 1 (tools/section_profile.py names them); one lane of a wave per id
#define ORLG_NSEC 20
#ifdef ORLG_SECTIONS
__device__ unsigned long long orlg_sections[ORLG_NSEC];
#define SEC_DECL_G __shared__ unsigned long long sec_acc[16][ORLG_NSEC]; long long sec_t0 = 0; int sec_cur = 0; \
    if (lane < ORLG_NSEC) sec_acc[wib][lane] = 0ull; wave_sync(); sec_t0 = __builtin_readcyclecounter();
#define SEC_DECL __shared__ unsigned long long sec_acc[ORLG_MAX_WAVES_PER_BLOCK][ORLG_NSEC]; long long sec_t0 = 0; int sec_cur = 0; \
    if (lane < ORLG_NSEC) sec_acc[wib][lane] = 0ull; wave_sync(); sec_t0 = __builtin_readcyclecounter();
#define SEC(i) do { const long long sec_n = __builtin_readcyclecounter(); if (lane == 0) sec_acc[wib][sec_cur] += (unsigned long long)(sec_n - sec_t0); \
    sec_t0 = sec_n; sec_cur = (i); } while (0)
#define SEC_FLUSH do { SEC(0); wave_sync(); if (lane < ORLG_NSEC) atomicAdd(&orlg_sections[lane], sec_acc[wib][lane]); } while (0)
// device functions that time their own sub-sections take the kernel's accumulators along
#define SEC_PARAMS , unsigned long long (*sec_acc)[ORLG_NSEC], long long &sec_t0, int &sec_cur, int wib
#define SEC_ARGS , sec_acc, sec_t0, sec_cur, wib
#else
#define SEC_PARAMS
#define SEC_ARGS
#define SEC_DECL
#define SEC_DECL_G
#define SEC(i) do { } while (0)
#define SEC_FLUSH do { } while (0)
#endif
