// Widest rows (elements) the LayerNorm entry points of norm.hip take: wider is M3AE_ERR_UNSUPPORTED before any launch.  xattn.hip
// answers m3ae_xattn_supported / m3ae_xattn_bwd_supported from the same numbers (it closes with these calls).
#pragma once

constexpr int LN_FWD_MAX_D = 4096;         // m3ae_layernorm_fwd: up to 16 chunks of 4 elements per lane
constexpr int LN_FWD_MIXED_MAX_D = 2048;   // m3ae_layernorm_fwd_mixed: what its backward takes (the kernel itself covers 4096)
constexpr int LN_BWD_MAX_D = 2048;         // every backward: the [4 waves][2][D] fp32 combine fills the 64 KiB of LDS at 2048
