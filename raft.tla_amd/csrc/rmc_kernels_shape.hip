// rmc_kernels_shape.hip — one packed shape's object (-DRMC_SHAPE_S=<servers> -DRMC_SHAPE_K=<bag
// slots>): its instantiations of the kernel templates behind its table of launchers, and its own
// __constant__ fingerprint salt (the table's set_salt).
#if !defined(RMC_SHAPE_S) || !defined(RMC_SHAPE_K)
#error "rmc_kernels_shape.hip builds one shape: -DRMC_SHAPE_S=<S> -DRMC_SHAPE_K=<K>"
#endif
#include "rmc_launch_shape.h"

namespace rmc {

#define RMC_SHAPE_TABLE_(SS, KK) RMC_SHAPE_TABLE(SS, KK)
extern const ShapeKernels RMC_SHAPE_TABLE_(RMC_SHAPE_S, RMC_SHAPE_K) = shape_table<RMC_SHAPE_S, RMC_SHAPE_K>();

}  // namespace rmc
