// Stand-in for the CUDA header of this name: the host execution layer (cuda_host.h).
#pragma once
#include "cuda_host.h"
