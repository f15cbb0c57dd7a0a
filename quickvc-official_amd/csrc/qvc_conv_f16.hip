// fp16-operand instantiation of the conv kernel (own translation unit so the two operand
// types compile in parallel).
#include "qvc_conv_impl.h"
#include "qvc_post_tail_impl.h"
namespace qvc { template int dispatch_conv<_Float16>(const LaunchChoice&, const ConvArgs&, void*);
template int dispatch_post_tail<_Float16>(const LaunchChoice&, const PostTailArgs&, void*);
template int dispatch_wn_stack<_Float16>(const LaunchChoice&, const WnStackArgs&, void*);
template int dispatch_wn<_Float16>(const LaunchChoice&, const WnArgs&, void*);
template int dispatch_pair<_Float16, _Float16>(const LaunchChoice&, const PairArgs3&, void*); }
#ifdef QVC_SATCOUNT
namespace qvc { QVC_SAT_READER(sat_count_conv_f16) }
#endif
