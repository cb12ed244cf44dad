// gemx_inst.hip -- ONE kernel unit: every stepping kernel of one (system, converter unit, dtype), built as its own shared object
//   hipcc -DGEMX_INST_SYS=<0..7> -DGEMX_INST_CONV=<0..11> -DGEMX_INST_F64=<0|1> -shared gemx_inst.hip -o libgemx_u<S>_<C>_<F>.so
// (gym_electric_motor_amd/build.py builds the 38 units in parallel) and loaded by gemx_create with dlopen (gemx_capi.hip: load_unit): a
// handle maps libgemx.so and the one unit it runs.  A unit links nothing of libgemx.so: its error messages go through the sink
// gemx_unit_init receives (gemx_unit_host.hpp).
#include "gemx_kernels.hpp"
#include "gemx_unit_host.hpp"

#if !defined(GEMX_INST_SYS) || !defined(GEMX_INST_CONV) || !defined(GEMX_INST_F64)
#error "define GEMX_INST_SYS, GEMX_INST_CONV and GEMX_INST_F64"
#endif

namespace gemx {
#if GEMX_INST_F64
using InstReal = double;
#else
using InstReal = float;
#endif
}  // namespace gemx

extern "C" {
__attribute__((visibility("default"))) int gemx_unit_init(unsigned long long handle_bytes, int abi, void (*set_error)(const char *)) {
    return gemx::unit_init(handle_bytes, abi, set_error);
}
__attribute__((visibility("default"))) int gemx_unit_launch(gemx_handle *h, const gemx::RolloutCall &call, hipStream_t st) {
    return gemx::launch_advance_unit<GEMX_INST_SYS, GEMX_INST_CONV, gemx::InstReal>(h, call, st);
}
}
