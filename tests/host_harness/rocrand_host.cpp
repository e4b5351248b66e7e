// rocrand_host.cpp -- rocRAND's own Philox4x32-10 device engine compiled for the HOST (its functions are __host__ __device__): the engine
// tests/rng_oracle.py is held to.  extern "C" wrappers only; nothing of csrc/ is included.  TEST HARNESS ONLY.
// Build: g++ -D__HIP_PLATFORM_AMD__ -I<rocm>/include (tests/test_rng_oracle_host.py, through build_so).
#include <cstdio>   // (rocrand_mtgp32.h, which rocrand_kernel.h pulls in, calls printf without including it)
#include <hip/hip_runtime.h>
#include <rocrand/rocrand_kernel.h>

extern "C" {

// `n` draws from rocrand_init(seed, subseq, offset); ops[j]: 0 = rocrand (raw word), 1 = rocrand_uniform, 2 = rocrand_normal.
// words[j] receives the raw word (op 0), values[j] the float (ops 1, 2).  Returns 0, or -1 for an unknown op.
int rr_draws(unsigned long long seed, unsigned long long subseq, unsigned long long offset, int n, const int* ops, unsigned* words, float* values) {
  rocrand_state_philox4x32_10 st;
  rocrand_init(seed, subseq, offset, &st);
  for (int j = 0; j < n; j++) {
    words[j] = 0u; values[j] = 0.0f;
    if (ops[j] == 0) words[j] = rocrand(&st);
    else if (ops[j] == 1) values[j] = rocrand_uniform(&st);
    else if (ops[j] == 2) values[j] = rocrand_normal(&st);
    else return -1;
  }
  return 0;
}

// the conversion alone: rocrand_uniform's expression on a given word
float rr_uniform_of(unsigned w) { return rocrand_device::detail::uniform_distribution(w); }

}  // extern "C"
