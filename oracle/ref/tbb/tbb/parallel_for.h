/* A serial stand-in for the one oneTBB call the map generator makes:
 * parallel_for(first, last, f) runs f(i) for i in [first, last), in order.
 * Test infrastructure only (oracle/Makefile, the `ref` targets). */
#ifndef VXREF_TBB_PARALLEL_FOR_H
#define VXREF_TBB_PARALLEL_FOR_H
namespace tbb {
template <class Index, class Function>
void parallel_for(Index first, Index last, const Function &f) {
    for (Index i = first; i < last; ++i) f(i);
}
}  // namespace tbb
#endif
