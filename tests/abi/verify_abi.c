/* include/sgpu.h is still plain C, and declares the verify chain: the parameter struct with its
 * fields, the defaults function and both entry points with their exact prototypes.  Compiled as
 * C to an object file only (tests/test_verify_abi.py: gcc -std=c99 -pedantic-errors -Werror -c),
 * so every check here is a compile-time one and no library is needed. */
#include <stddef.h>

#include "sgpu.h"

typedef void (*defaults_fn)(sgpu_verify_params*);
typedef int (*verify_batch_fn)(sgpu_ctx*, const uint8_t*, const float*, const int64_t*, int,
                               const int*, int, const sgpu_verify_params*, float*, int*, float*,
                               int*, int*, int*, int64_t, int*, int);
typedef int (*verify_images_fn)(sgpu_ctx*, const int*, int, const sgpu_verify_params*, float*,
                                int*, float*, int*, int*, int*, int64_t, int*);

/* an initialisation from an incompatible function-pointer type is an error under -Werror */
defaults_fn verify_abi_defaults = sgpu_default_verify_params;
verify_batch_fn verify_abi_batch = sgpu_verify_batch;
verify_images_fn verify_abi_images = sgpu_verify_images;

/* eleven 4-byte fields, no padding: the layout python/sgpu_types.py mirrors (a negative array
 * size where one of them fails) */
typedef char verify_abi_size[sizeof(sgpu_verify_params) == 44 ? 1 : -1];
typedef char verify_abi_h_threshold[offsetof(sgpu_verify_params, h_threshold) == 16 ? 1 : -1];
typedef char verify_abi_seed[offsetof(sgpu_verify_params, seed) == 36 ? 1 : -1];
typedef char verify_abi_rounds[offsetof(sgpu_verify_params, refine_rounds) == 40 ? 1 : -1];

int verify_abi_fields(void) {
    sgpu_verify_params p;
    p.distmax = 0.7f;
    p.ratiomax = 0.8f;
    p.mutual_best_match = 1;
    p.max_match = 4096;
    p.h_threshold = 2.0f;
    p.f_threshold = 4.0f;
    p.hdistmax = 2.0f;
    p.fdistmax = 4.0f;
    p.iterations = 512;
    p.seed = 0u;
    p.refine_rounds = 3;
    return p.mutual_best_match + p.max_match + p.iterations + (int)p.seed + p.refine_rounds;
}
