// switches.hip -- the table of behaviour switches (include/madeleine_amd.h, "Behaviour switches") and the mdl_switch_* entry points.
// The only place of the library that reads the environment: once, when the table is built.  Host only.
#include <stdlib.h>

#include <atomic>

#include "switches.hpp"

namespace mdl {
namespace {

enum Kind { PRESENCE, INTEGER };

struct Switches {
    const char* name[MDL_SW_COUNT] = {};
    std::atomic<int64_t> value[MDL_SW_COUNT];

    // PRESENCE: 1 when the variable exists, whatever its text; INTEGER: atoll of the text, the default without the variable
    void row(int id, const char* env, Kind kind, int64_t dflt) {
        const char* text = getenv(env);
        name[id] = env;
        value[id].store(kind == PRESENCE ? (text != nullptr) : (text ? atoll(text) : dflt), std::memory_order_relaxed);
    }
    Switches() {
        row(MDL_SW_INFONCE_FUSED, "MADELEINE_INFONCE_FUSED", PRESENCE, 0);
        row(MDL_SW_BF16_GATE128, "MADELEINE_BF16_GATE128", PRESENCE, 0);
        row(MDL_SW_DROP_16BIT, "MADELEINE_DROP_16BIT", PRESENCE, 0);
        row(MDL_SW_GOT_NO192, "MADELEINE_GOT_NO192", PRESENCE, 0);
        row(MDL_SW_GOT_NOSPLIT, "MADELEINE_GOT_NOSPLIT", PRESENCE, 0);
        row(MDL_SW_GOT_NO_HALF_PRODUCTS, "MADELEINE_GOT_NO_HALF_PRODUCTS", PRESENCE, 0);
        row(MDL_SW_BF16_GATE_PERSIST, "MADELEINE_BF16_GATE_PERSIST", INTEGER, MDL_GATE_BF16_PMODE);
        row(MDL_SW_GATE_PERSIST, "MADELEINE_GATE_PERSIST", INTEGER, MDL_GATE_SP_PMODE);
        row(MDL_SW_BF16_LIN_PERSIST, "MADELEINE_BF16_LIN_PERSIST", INTEGER, 1);
        row(MDL_SW_BF16_LIN256_MINK, "MADELEINE_BF16_LIN256_MINK", INTEGER, 512);
        row(MDL_SW_BF16_TN256, "MADELEINE_BF16_TN256", INTEGER, 1);
        row(MDL_SW_SPLIT_TOKENS, "MADELEINE_SPLIT_TOKENS", INTEGER, MDL_SPLIT_TOKENS);
        row(MDL_SW_SP_NT_STAGES, "MADELEINE_SP_NT_STAGES", INTEGER, MDL_SP_NT_STAGES);
        row(MDL_SW_SP_TN_STAGES, "MADELEINE_SP_TN_STAGES", INTEGER, MDL_SP_TN_STAGES);
        row(MDL_SW_BF16_STAGES, "MADELEINE_BF16_STAGES", INTEGER, MDL_BF16_STAGES);
        row(MDL_SW_BF16_LIN_STAGES, "MADELEINE_BF16_LIN_STAGES", INTEGER, MDL_BF16_LIN_STAGES);
    }
};
// handed out by a function (a table at namespace scope would be emitted into the device code as well, got_host.hpp); the function-local
// static is what makes the one read of the environment thread-safe
Switches& switches() {
    static Switches s;
    return s;
}

// the calling thread's overrides: bit id of `mask` says that value[id] holds one
struct Override {
    int64_t value[MDL_SW_COUNT];
    uint32_t mask;
};
static_assert(MDL_SW_COUNT <= 32, "one mask bit per switch");
thread_local Override override_tl = {};

bool bad_id(int id) { return id < 0 || id >= MDL_SW_COUNT; }

}  // namespace

int64_t sw(int id) {
    const Override& o = override_tl;
    return (o.mask >> id & 1u) ? o.value[id] : switches().value[id].load(std::memory_order_relaxed);
}

}  // namespace mdl

using namespace mdl;

extern "C" int mdl_switch_get(int id, int64_t* value) {
    if (bad_id(id) || !value) return MDL_E_ARG;
    *value = sw(id);
    return MDL_OK;
}
extern "C" int mdl_switch_set(int id, int64_t value) {
    if (bad_id(id)) return MDL_E_ARG;
    switches().value[id].store(value, std::memory_order_relaxed);
    return MDL_OK;
}
extern "C" int mdl_switch_set_thread(int id, int64_t value) {
    if (bad_id(id)) return MDL_E_ARG;
    override_tl.value[id] = value;
    override_tl.mask |= 1u << id;
    return MDL_OK;
}
extern "C" int mdl_switch_clear_thread(int id) {
    if (bad_id(id)) return MDL_E_ARG;
    override_tl.mask &= ~(1u << id);
    return MDL_OK;
}
extern "C" const char* mdl_switch_name(int id) { return bad_id(id) ? nullptr : switches().name[id]; }
