// part of oracle/cuda_host_shim: every CUDA / OptiX name the reference's include chain needs is in cuda_runtime.h
#pragma once
#include "cuda_runtime.h"
