/* include/sgpu.h is still plain C, and declares the pose calls with their exact prototypes.
 * Compiled as C to an object file only (tests/test_pose.py: gcc -std=c99 -pedantic-errors -Wall
 * -Werror -c), so every check here is a compile-time one and no library is needed. */
#include "sgpu.h"

typedef int (*pose_batch_fn)(sgpu_ctx*, const float*, const int64_t*, int, const float*, const int*,
                             int, const int*, const int*, const float*, float, float, float*,
                             float*, int*, uint8_t*, float*, int);
typedef int (*pose_images_fn)(sgpu_ctx*, const float*, const int*, int, const int*, const int*,
                              const float*, float, float, float*, float*, int*, uint8_t*, float*);

/* an initialisation from an incompatible function-pointer type is an error under -Werror */
pose_batch_fn pose_abi_batch = sgpu_pose_batch;
pose_images_fn pose_abi_images = sgpu_pose_images;
