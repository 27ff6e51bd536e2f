// ABI version of libmqdet_hip.so (see include/mqdet_hip.h).  It changes when an existing argument list changes; entry points that were only
// added (the evaluators, mq_tta_merge_special / mq_tta_merge_finalize_special, mq_tta_merge_nms) leave it where it is: ops.load_library resolves every name.
#include "../../include/mqdet_hip.h"
extern "C" int mq_abi_version(void) { return 31; }
