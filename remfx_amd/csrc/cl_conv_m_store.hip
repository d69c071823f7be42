// rfx_cl_conv, epilogue mode RFX_CL_STORE (kernel template: csrc/cl_conv.h)
#include "cl_conv.h"

int cl_conv_mode_store(const ClConvK& k, dim3 grid, hipStream_t s, bool query) { return cl_conv_dispatch<RFX_CL_STORE>(k, grid, s, query); }
