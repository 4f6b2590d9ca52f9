// host/host_common.hpp — what the host layer's translation units share (private to the library).
#pragma once

#include <cstdio>
#include <cstdlib>

// prosper keeps its asserts in every build type (readme.md:88-92): programmer errors abort.
#define PROSPER_ASSERT(cond)                                                                                           \
    do                                                                                                                 \
    {                                                                                                                  \
        if (!(cond))                                                                                                   \
        {                                                                                                              \
            std::fprintf(stderr, "%s:%d: assertion failed: %s\n", __FILE__, __LINE__, #cond);                          \
            std::abort();                                                                                              \
        }                                                                                                              \
    } while (0)

// the plain-C shims' last error (prosper_host_last_error); defined in rt_reference.cpp
extern "C" void prosper_host_set_error(const char *message);
