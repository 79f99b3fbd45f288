// Error strings / ABI version of libuniir_hip.so (include/uniir_hip.h).
#include "../../include/uniir_hip.h"

extern "C" const char* uniir_strerror(int code) {
    switch (code) {
        case UNIIR_OK: return "ok";
        case UNIIR_EINVAL: return "invalid argument (null pointer, negative size or bad enum)";
        case UNIIR_ESHAPE: return "shape not supported by the gfx950 kernels";
        case UNIIR_EALIGN: return "pointer or leading dimension is not 16-byte aligned";
        case UNIIR_ELAUNCH: return "HIP kernel launch failed";
        case UNIIR_EUNSUPPORTED: return "unsupported configuration";
        default: return "unknown uniir error code";
    }
}
// 2 (round 6): uniir_clip_tower grew pool_last_block; uniir_gemm_timing_read_ex returns the fallback flag; new entry points
// uniir_reduce_scratch, uniir_attention_{fwd,bwd}_rows, uniir_dropout_{f32,bf16}_rows, uniir_gemm_timing_filter
// 4: new entry point uniir_reduce_stats
// 5: new entry points uniir_image_batch_plan, uniir_image_preprocess_batch (uniir_image_desc / _plan / _batch_info)
// 6: new entry points uniir_attention_fwd_long, uniir_attention_bwd_long
// 7: new entry points uniir_attn_rel_fwd_f16, uniir_attn_rel_fwd_long_f16, uniir_rmsnorm_fwd_f16; still 7: uniir_attn_f32_rel_fwd
// still 7: uniir_clip_tower grew ln_bwd_side (after splitk_ws_bytes, in front of the flags that end the struct); new entry points
// uniir_gemm_wgrad_ln_bwd, uniir_gemm_wgrad_side_plan -- a binding of this header fails to load an older library on those symbols
extern "C" int uniir_abi_version(void) { return 7; }
