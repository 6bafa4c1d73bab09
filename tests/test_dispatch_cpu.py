"""csrc/dispatch.h alone, built with the host compiler: run-time switches reach the lambda as constants, in argument order."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAIN = r"""
#include "dispatch.h"
#include <cstdio>

int main()
{
    int bad = 0;
    // five switches, all 2^5 inputs: the constants equal the run-time values, in argument order
    for (int v = 0; v < 32; ++v) {
        const bool b[5] = {(v & 1) != 0, (v & 2) != 0, (v & 4) != 0, (v & 8) != 0, (v & 16) != 0};
        int calls = 0;
        const int got = lbmpm::dispatch([&](auto a0, auto a1, auto a2, auto a3, auto a4) {
            ++calls;
            constexpr bool k[5] = {decltype(a0)::value, decltype(a1)::value, decltype(a2)::value, decltype(a3)::value, decltype(a4)::value};
            int w = 0;
            for (int i = 0; i < 5; ++i) w |= (k[i] ? 1 : 0) << i;
            return w;
        }, b[0], b[1], b[2], b[3], b[4]);
        if (got != v || calls != 1) { std::printf("dispatch: switches %d arrived as %d in %d calls\n", v, got, calls); ++bad; }
    }
    // no switch: f()
    if (lbmpm::dispatch([] { return 7; }) != 7) { std::printf("dispatch without a switch\n"); ++bad; }
    // the tracer count: 1..4, anything else is 4
    const int in[6] = {0, 1, 2, 3, 4, 5}, want[6] = {4, 1, 2, 3, 4, 4};
    for (int i = 0; i < 6; ++i) {
        int calls = 0;
        const int got = lbmpm::dispatch_int<1, 4>([&](auto n) { ++calls; constexpr int k = decltype(n)::value; return k; }, in[i]);
        if (got != want[i] || calls != 1) { std::printf("dispatch_int<1, 4>(%d) arrived as %d in %d calls, not %d\n", in[i], got, calls, want[i]); ++bad; }
    }
    return bad ? 1 : 0;
}
"""


def test_dispatch_header_with_the_host_compiler():
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.cpp"), "w") as f:
            f.write(MAIN)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "openlbmpm_amd", "csrc"), "-o", os.path.join(d, "t"),
                               os.path.join(d, "t.cpp")])
        run = subprocess.run([os.path.join(d, "t")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0, run.stdout.decode()
