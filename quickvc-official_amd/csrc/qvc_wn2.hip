// The continuous-stream WaveNet stack kernel (qvc_wn2_impl.h), both operand types: a translation unit of its own so
// that it compiles beside the conv kernels.
#include "qvc_wn2_impl.h"
namespace qvc {
template int dispatch_wn_stack2<_Float16>(const LaunchChoice&, const WnStackArgs&, void*);
template int dispatch_wn_stack2<__bf16>(const LaunchChoice&, const WnStackArgs&, void*);
}  // namespace qvc
#ifdef QVC_SATCOUNT
namespace qvc { QVC_SAT_READER(sat_count_wn2) }
#endif
