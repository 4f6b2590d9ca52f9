// pt_error.hpp — how the library's translation units report a failure (private).
#pragma once

#include <hip/hip_runtime_api.h>

#include <string>

#include "../../include/prosper_pt/prosper_pt.h"

namespace ppt
{
// records `msg` as the calling thread's last error (prosper_pt_last_error) and returns `code`
int fail(int code, const std::string &msg);
} // namespace ppt

#define PPT_HIP(call)                                                                                                  \
    do                                                                                                                 \
    {                                                                                                                  \
        const hipError_t e_ = (call);                                                                                  \
        if (e_ != hipSuccess)                                                                                          \
            return ppt::fail(PROSPER_PT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));                   \
    } while (0)
