// The finish kernels' arithmetic on the host, for tests/test_finish_bits_cpu.py: reads from stdin a uint64 count, a uint64 number
// of steps, count floats a, count floats v and the steps h as doubles; writes, per step, the count floats
// (float)__builtin_fma((double)a, h, (double)v) -- the expression of update_kernel, kdk_kick_kernel and kdk_kick_drift_kernel.
#include <cstdint>
#include <cstdio>
#include <vector>

int main()
{
    uint64_t count = 0, steps = 0;
    if (std::fread(&count, sizeof count, 1, stdin) != 1 || std::fread(&steps, sizeof steps, 1, stdin) != 1)
        return 1;
    std::vector<float> a(count), v(count), out(count);
    std::vector<double> h(steps);
    if (std::fread(a.data(), sizeof(float), count, stdin) != count || std::fread(v.data(), sizeof(float), count, stdin) != count ||
        std::fread(h.data(), sizeof(double), steps, stdin) != steps)
        return 1;
    for (uint64_t s = 0; s < steps; ++s) {
        for (uint64_t i = 0; i < count; ++i)
            out[i] = (float)__builtin_fma((double)a[i], h[s], (double)v[i]);
        if (std::fwrite(out.data(), sizeof(float), count, stdout) != count)
            return 1;
    }
    return 0;
}
