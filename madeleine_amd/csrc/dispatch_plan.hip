// dispatch_plan.hip -- mdl_dispatch_plan (include/madeleine_amd.h): what a launcher would choose for a shape, asked of the launcher's own
// selection functions in its translation unit.  Host only: no device, no device memory.
#include "common.hpp"

namespace mdl {
int plan_gate_fp32_bwd(int64_t T, int H, int64_t* o);                // abmil_gate.hip
int plan_gate_split(int product, int64_t T, int H, int64_t* o);      // abmil_gate_split.hip
int plan_gate_bf16(int product, int64_t T, int H, int64_t* o);       // abmil_gate_bf16.hip
int plan_split_tn(int64_t T, int Mi, int N, int64_t* o);             // split_gemm.hip
int plan_linear_fp32_bwd(int64_t T, int N, int K, int64_t* o);       // linear_fp32.hip
int plan_linear_bf16(int product, int64_t T, int N, int K, int64_t* o);   // linear_bf16.hip
int plan_got(int64_t k, int n, int cus, int64_t* o);                 // got.hip
int plan_infonce_neg(int64_t N, int M, int D, int64_t* o);           // infonce.hip
int plan_got_tiled(int64_t k, int n, int m, int d, int64_t* o);      // got_tiled.hip
}  // namespace mdl

using namespace mdl;

extern "C" int mdl_dispatch_plan(int product, int64_t T, int a, int b, int cus, int64_t* out_host, int n_out) {
    if (!out_host || n_out < 1 || T < 0) return MDL_E_ARG;
    int64_t o[MDL_PLAN_FIELDS] = {};
    int rc;
    switch (product) {
    case MDL_PLAN_GATE_FP32_BWD:
        rc = (a < 1 || a > MDL_MAX_HEADS) ? MDL_E_ARG : plan_gate_fp32_bwd(T, a, o);
        break;
    case MDL_PLAN_GATE_SPLIT_FWD:
    case MDL_PLAN_GATE_SPLIT_BWD:
        rc = (a < 1 || a > MDL_MAX_HEADS) ? MDL_E_ARG : plan_gate_split(product, T, a, o);
        break;
    case MDL_PLAN_GATE_BF16_FWD:
    case MDL_PLAN_GATE_BF16_BWD:
        rc = (a < 1 || a > MDL_MAX_HEADS) ? MDL_E_ARG : plan_gate_bf16(product, T, a, o);
        break;
    case MDL_PLAN_SPLIT_TN: rc = plan_split_tn(T, a, b, o); break;
    case MDL_PLAN_LINEAR_FP32_BWD: rc = plan_linear_fp32_bwd(T, a, b, o); break;
    case MDL_PLAN_LINEAR_BF16_FWD:
    case MDL_PLAN_LINEAR_BF16_BWD: rc = plan_linear_bf16(product, T, a, b, o); break;
    case MDL_PLAN_GOT: rc = plan_got(T, a, cus, o); break;
    case MDL_PLAN_INFONCE_NEG: rc = plan_infonce_neg(T, a, b, o); break;
    case MDL_PLAN_GOT_TILED: rc = plan_got_tiled(T, a, a, b, o); break;
    case MDL_PLAN_GOT_TILED_RECT: rc = plan_got_tiled(T, a, b, 1, o); break;   // a = n, b = m; no field depends on d
    default: rc = MDL_E_ARG;
    }
    if (rc) return rc;
    for (int i = 0; i < n_out; ++i) out_host[i] = i < MDL_PLAN_FIELDS ? o[i] : 0;
    return MDL_OK;
}
