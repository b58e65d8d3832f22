// Host build of csrc/augment_math.h for tests/test_augment_cpu.py: the text the device kernel compiles, callable on host
// arrays, so that the scalar augmentation arithmetic is checked against the reference fixture without a GPU.
#include "augment_math.h"

extern "C" void augment_host(const fpd_augment_t* a, int b, int i, fpd_aug_sample_t* out) { fpd_augment_sample(*a, b, i, *out); }
extern "C" int augment_host_sizeof(void) { return (int)sizeof(fpd_aug_sample_t); }
