/* include/sgpu.h is still plain C, and declares the track builder: the two calls with their exact
 * prototypes and the two row verdicts.  Compiled as C to an object file only (tests/test_tracks.py:
 * gcc -std=c99 -pedantic-errors -Wall -Werror -c), so every check here is a compile-time one and no
 * library is needed. */
#include "sgpu.h"

typedef int (*tracks_batch_fn)(sgpu_ctx*, const int64_t*, int, const int*, int, const int*,
                               const int*, int, int*, int64_t*, int*, long long*);
typedef int (*tracks_images_fn)(sgpu_ctx*, const int*, int, const int*, const int*, int, int*,
                                int64_t*, int*, long long*);

/* an initialisation from an incompatible function-pointer type is an error under -Werror */
tracks_batch_fn tracks_abi_batch = sgpu_tracks_batch;
tracks_images_fn tracks_abi_images = sgpu_tracks_images;

/* a negative array size is an error */
typedef char tracks_abi_none[SGPU_TRACK_NONE == -1 ? 1 : -1];
typedef char tracks_abi_inconsistent[SGPU_TRACK_INCONSISTENT == -2 ? 1 : -1];
