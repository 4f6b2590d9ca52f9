// tests/texture_readback_main.cpp — render::TextureReadback (csrc/host/texture_readback.cpp) on a CPU against fakes of
// the two library calls it sits on: the reference's m_framesUntilReady over MAX_FRAMES_IN_FLIGHT = 2, its three
// assertions as exceptions, and a copy that has not finished when the frames have.  Prints "ok" and returns 0.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../prosper_amd/csrc/host/texture_readback.hpp"

namespace
{
int g_records = 0;      // prosper_pt_texture_readback calls
bool g_refuse = false;  // ... the next one is refused
bool g_landed = false;  // the copy has finished
float g_value[4] = {0.25f, 0.0f, 0.0f, 1.0f};
std::string g_error;
} // namespace

extern "C" {
struct prosper_pt_ctx
{
    int unused;
};
int prosper_pt_texture_readback(prosper_pt_ctx *, uint32_t, float, float, void *)
{
    if (g_refuse) return PROSPER_PT_ERR_NO_SCENE;
    ++g_records;
    return PROSPER_PT_OK;
}
int prosper_pt_try_texture_readback(prosper_pt_ctx *, float out[4])
{
    if (!g_landed) return PROSPER_PT_NOT_READY;
    std::memcpy(out, g_value, sizeof(g_value));
    g_landed = false;
    return PROSPER_PT_OK;
}
const char *prosper_pt_last_error(void) { return "refused by the fake"; }
void prosper_host_set_error(const char *message) { g_error = message; }
}

#define CHECK(cond)                                                                                                    \
    do                                                                                                                 \
    {                                                                                                                  \
        if (!(cond))                                                                                                   \
        {                                                                                                              \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);                                            \
            return 1;                                                                                                  \
        }                                                                                                              \
    } while (0)

template <class F> static bool throws_logic(F f)
{
    try
    {
        f();
    }
    catch (const std::logic_error &)
    {
        return true;
    }
    return false;
}

int main()
{
    prosper_pt_ctx ctx = {};
    render::TextureReadback rb;
    rb.init(&ctx);
    CHECK(render::MAX_FRAMES_IN_FLIGHT == 2 && rb.framesUntilReady() == -1);
    CHECK(throws_logic([&] { (void)rb.readback(); })); // "No readback in flight"
    rb.startFrame();                                    // nothing queued: nothing to count
    CHECK(rb.framesUntilReady() == -1);

    rb.record(3, 7.0f, 8.0f, nullptr);
    CHECK(g_records == 1 && rb.framesUntilReady() == 2);
    CHECK(throws_logic([&] { rb.record(3, 1.0f, 1.0f, nullptr); })); // "Readback already queued and unread"
    CHECK(g_records == 1);
    g_landed = true; // the copy is there at once; the frames are not
    CHECK(!rb.readback().has_value());
    rb.startFrame();
    CHECK(rb.framesUntilReady() == 1 && !rb.readback().has_value());
    rb.startFrame();
    CHECK(rb.framesUntilReady() == 0);
    CHECK(throws_logic([&] { rb.startFrame(); })); // at 0 and nobody asked: "Forgot to call readback()"
    const auto value = rb.readback();
    CHECK(value.has_value() && (*value)[0] == 0.25f && (*value)[3] == 1.0f);
    CHECK(rb.framesUntilReady() == -1);
    CHECK(throws_logic([&] { (void)rb.readback(); })); // handed out once

    // a copy that has not landed when the frames have: empty, asked again the next frame
    rb.record(3, 1.0f, 1.0f, nullptr);
    rb.startFrame();
    rb.startFrame();
    CHECK(rb.framesUntilReady() == 0 && !rb.readback().has_value());
    rb.startFrame(); // polled at 0: no assertion
    CHECK(rb.framesUntilReady() == 0);
    g_landed = true;
    CHECK(rb.readback().has_value() && rb.framesUntilReady() == -1);

    // a refusal of the library leaves nothing queued
    g_refuse = true;
    bool refused = false;
    try
    {
        rb.record(3, 1.0f, 1.0f, nullptr);
    }
    catch (const std::runtime_error &e)
    {
        refused = std::string(e.what()).find("refused by the fake") != std::string::npos;
    }
    CHECK(refused && rb.framesUntilReady() == -1);
    std::puts("ok");
    return 0;
}
