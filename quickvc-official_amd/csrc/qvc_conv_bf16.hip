// bf16-operand instantiation of the conv kernel.
#include "qvc_conv_impl.h"
#include "qvc_post_tail_impl.h"
namespace qvc { template int dispatch_conv<__bf16>(const LaunchChoice&, const ConvArgs&, void*);
template int dispatch_post_tail<__bf16>(const LaunchChoice&, const PostTailArgs&, void*);
template int dispatch_wn_stack<__bf16>(const LaunchChoice&, const WnStackArgs&, void*);
template int dispatch_wn<__bf16>(const LaunchChoice&, const WnArgs&, void*);
template int dispatch_pair<__bf16, __bf16>(const LaunchChoice&, const PairArgs3&, void*);
// QVC_BF16X: bf16 operands, f16 residual stream
template int dispatch_pair<__bf16, _Float16>(const LaunchChoice&, const PairArgs3&, void*); }
#ifdef QVC_SATCOUNT
namespace qvc { QVC_SAT_READER(sat_count_conv_bf16) }
#endif
