// svx_wave_scan.hpp -- the wave's inclusive prefix sum in the vector ALU, shared by bgzf_tokens_kernel (svx_inflate2.hip) and
// bgzf_lz_table_kernel (svx_lz_table.hip).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace svx_wave {

// Inclusive prefix sum over the wave in the vector ALU (row shifts inside the rows of 16 lanes + the two row broadcasts of gfx9):
// seven data-parallel moves instead of six ds_bpermute round trips through the LDS crossbar (what __shfl_up compiles to here).
// Every lane of the wave must be active.
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)
{
    uint32_t r = v;
    r += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);      // row_shr:1
    r += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);      // row_shr:2
    r += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x113, 0xf, 0xf, true);      // row_shr:3
    r += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)r, 0x114, 0xf, 0xe, true);      // row_shr:4, banks 1-3
    r += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)r, 0x118, 0xf, 0xc, true);      // row_shr:8, banks 2-3
    r += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)r, 0x142, 0xa, 0xf, false);     // row_bcast:15 into rows 1 and 3
    r += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)r, 0x143, 0xc, 0xf, false);     // row_bcast:31 into rows 2 and 3
    return r;
}

}  // namespace svx_wave
