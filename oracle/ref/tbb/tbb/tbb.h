/* Stand-in umbrella header (see parallel_for.h). */
#ifndef VXREF_TBB_TBB_H
#define VXREF_TBB_TBB_H
#include "parallel_for.h"
#include "blocked_range3d.h"
#endif
