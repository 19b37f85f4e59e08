// rvcx kernel launchers (internal; the public C-ABI is include/rvcx.h): every stage's header, for the runtime and the
// measurement binaries. A kernel file includes its own stage's header instead.
#pragma once
#include "attention_kernels.h"
#include "conv_kernels.h"
#include "crepe_kernels.h"
#include "fcpe_kernels.h"
#include "fe_kernels.h"
#include "ivf_kernels.h"
#include "kernel_base.h"
#include "pipeline_kernels.h"
#include "resample_kernels.h"
#include "rowops_kernels.h"
#include "stream_kernels.h"
#include "vocoder_kernels.h"
