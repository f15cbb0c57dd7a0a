// The chained-ResBlock kernel (qvc_chain_impl.h) for the three operand / stream type combinations: a translation unit
// of its own so that it compiles beside the conv kernels.
#include "qvc_chain_impl.h"
namespace qvc {
template int dispatch_chain<_Float16, _Float16>(const LaunchChoice&, const ChainArgs&, void*);
template int dispatch_chain<__bf16, __bf16>(const LaunchChoice&, const ChainArgs&, void*);
template int dispatch_chain<__bf16, _Float16>(const LaunchChoice&, const ChainArgs&, void*);
}  // namespace qvc
#ifdef QVC_SATCOUNT
namespace qvc { QVC_SAT_READER(sat_count_chain) }
#endif
