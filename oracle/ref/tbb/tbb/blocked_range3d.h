/* Stand-in header: the generator includes it and uses nothing from it. */
#ifndef VXREF_TBB_BLOCKED_RANGE3D_H
#define VXREF_TBB_BLOCKED_RANGE3D_H
#endif
