// bgzf_fields_kernel.hip -- the field parse's two instantiations of the device deflate encoder's block kernel (bgzf_block_kernel.h; tuning
// key "bgzf_parse" = 1, docs/BGZF_FIELDS.md): with the fixed code and with a code of the block's own.  Built without machine LICM, as
// bgzf_dynamic_kernel.hip is, whose launch_bgzf_blocks_other launches them.
#include "bgzf_block_kernel.h"

namespace bvc {

template __global__ void bgzf_block_kernel<true, false>(const uint8_t *, const BlockDesc *, int64_t, uint8_t *, uint32_t *, uint32_t *, uint32_t);
template __global__ void bgzf_block_kernel<true, true>(const uint8_t *, const BlockDesc *, int64_t, uint8_t *, uint32_t *, uint32_t *, uint32_t);

#ifdef BVC_CHECK_LDS
BVC_DEFINE_DEBUG_READER(debug_read_bgzf_fields)
#endif

}  // namespace bvc
