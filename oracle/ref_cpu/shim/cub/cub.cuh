/* Stand-in for the CUDA toolkit header of this name: everything lives in refcpu.h. */
#pragma once
#include "../refcpu.h"
