// switches.hpp -- the behaviour switches of the library (include/madeleine_amd.h, "Behaviour switches"): mdl::sw(id) is the only way a
// launcher asks for one.  The table (id, environment name, default, kind), its storage and the mdl_switch_* entry points live in
// switches.hip; the environment is read there, once, and nowhere else.  Host only.
#pragma once
#include <stdint.h>

#include "../../include/madeleine_amd.h"

// The defaults of the integer switches that a build may override (-DMDL_...=n).  What a value means stays with its consumer.
#ifndef MDL_SP_NT_STAGES
#define MDL_SP_NT_STAGES 3      // split_engine.hpp: stages of the NT main loop's A ring
#endif
#ifndef MDL_SP_TN_STAGES
#define MDL_SP_TN_STAGES 3      // split_engine.hpp: the TN (dW) loops
#endif
#ifndef MDL_BF16_STAGES
#define MDL_BF16_STAGES 3       // tile_engine_bf16.hpp: the gate products
#endif
#ifndef MDL_BF16_LIN_STAGES
#define MDL_BF16_LIN_STAGES 31  // tile_engine_bf16.hpp: the Linear products (3 with the one-barrier NT loop)
#endif
#ifndef MDL_SPLIT_TOKENS
#define MDL_SPLIT_TOKENS 32768  // gate_common.hpp: tokens per split of the dW-type contractions
#endif
#ifndef MDL_GATE_BF16_PMODE
#define MDL_GATE_BF16_PMODE 1   // abmil_gate_bf16.hip: persistent mode of the 256-tile gate forward
#endif
#ifndef MDL_GATE_SP_PMODE
#define MDL_GATE_SP_PMODE 0     // abmil_gate_split.hip: persistent mode of the split gate forward
#endif

namespace mdl {

// The value of switch `id` (an MDL_SW_* of the header) as the calling thread sees it: its own override where one is set
// (mdl_switch_set_thread), the process value otherwise.  Two relaxed loads; no environment read after the first call of the process.
int64_t sw(int id);

}  // namespace mdl
