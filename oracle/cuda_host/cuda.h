// Stand-in for the CUDA driver header: the host execution layer (cuda_host.h).
#pragma once
#define CUDA_VERSION 2030
#include "cuda_host.h"
