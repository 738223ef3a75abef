/* include/sgpu.h is still plain C, and declares preemptive matching: the two selection calls and
 * the two pre-pass calls with their exact prototypes.  Compiled as C to an object file only
 * (tests/test_select.py: gcc -std=c99 -pedantic-errors -Wall -Werror -c), so every check here is a
 * compile-time one and no library is needed. */
#include "sgpu.h"

typedef int (*select_batch_fn)(sgpu_ctx*, const float*, int, const int64_t*, int, int, int*,
                               int64_t*, int);
typedef int (*select_images_fn)(sgpu_ctx*, int, int*, int64_t*);
typedef int (*prematch_batch_fn)(sgpu_ctx*, const uint8_t*, const float*, int, const int64_t*, int,
                                 const int*, int, int, float, float, int, int*, int*, int64_t, int);
typedef int (*prematch_images_fn)(sgpu_ctx*, const int*, int, int, float, float, int, int*, int*,
                                  int64_t);

/* an initialisation from an incompatible function-pointer type is an error under -Werror */
select_batch_fn prematch_abi_select_batch = sgpu_select_top_scale_batch;
select_images_fn prematch_abi_select_images = sgpu_select_top_scale_images;
prematch_batch_fn prematch_abi_batch = sgpu_prematch_batch;
prematch_images_fn prematch_abi_images = sgpu_prematch_images;
