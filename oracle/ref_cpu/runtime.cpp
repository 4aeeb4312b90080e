/*
 * runtime.cpp -- the execution model behind refcpu.h (TEST INFRASTRUCTURE ONLY; own code).
 *
 * A launch runs its blocks one after another on the calling OS thread, first to last or, with refcpu::reverse_blocks, last to first.  The
 * threads of a block are ucontext fibers.  The scheduler resumes them in rank order; a fiber runs until it returns or reaches a barrier, where
 * it yields back.  After one pass every live fiber stands at the same barrier (the reference's kernels reach every barrier with all threads of
 * the block), so the next pass is the code after it.  threadIdx is set on every switch; blockIdx once per block.
 */
#include <ucontext.h>

#include "shim/refcpu.h"

uint3 threadIdx, blockIdx;
dim3 blockDim, gridDim;

namespace refcpu {
bool reverse_blocks = false;
bool tex_quant = false;

namespace {
/* renderCUDA keeps a few hundred bytes of local arrays and calls glm and libm; 256 KiB per fiber leaves two orders of magnitude of headroom */
const size_t STACK = 256 * 1024;
struct Fiber { ucontext_t ctx; bool done; };
ucontext_t sched;
std::vector<Fiber> fibers;
std::vector<char> stacks;
void (*cur_body)(void*);
void* cur_arg;
int cur;           /* rank of the running fiber */
int count_acc;     /* predicates summed at the barrier being gathered */
int count_result;  /* sum of the barrier just completed */

void trampoline()
{
    cur_body(cur_arg);
    fibers[cur].done = true;
    swapcontext(&fibers[cur].ctx, &sched);
}
} // namespace

void barrier()
{
    swapcontext(&fibers[cur].ctx, &sched);
}

int barrier_count(int pred)
{
    count_acc += pred ? 1 : 0;
    swapcontext(&fibers[cur].ctx, &sched);
    return count_result;
}

void run_grid(dim3 grid, dim3 block, void (*body)(void*), void* arg)
{
    const int nthreads = (int)(block.x * block.y * block.z);
    const long nblocks = (long)grid.x * grid.y * grid.z;
    if (nthreads <= 0 || nblocks <= 0) return;
    if ((int)fibers.size() < nthreads) { fibers.resize(nthreads); stacks.resize((size_t)nthreads * STACK); }
    gridDim = grid; blockDim = block;
    cur_body = body; cur_arg = arg;
    for (long bi = 0; bi < nblocks; bi++) {
        const long b = reverse_blocks ? nblocks - 1 - bi : bi;
        blockIdx = uint3{(unsigned)(b % grid.x), (unsigned)((b / grid.x) % grid.y), (unsigned)(b / ((long)grid.x * grid.y))};
        for (int t = 0; t < nthreads; t++) {
            getcontext(&fibers[t].ctx);
            fibers[t].ctx.uc_stack.ss_sp = stacks.data() + (size_t)t * STACK;
            fibers[t].ctx.uc_stack.ss_size = STACK;
            fibers[t].ctx.uc_link = &sched;
            fibers[t].done = false;
            makecontext(&fibers[t].ctx, trampoline, 0);
        }
        count_acc = 0;
        for (int live = nthreads; live > 0;) {
            live = 0;
            for (int t = 0; t < nthreads; t++) {
                if (fibers[t].done) continue;
                cur = t;
                threadIdx = uint3{(unsigned)(t % block.x), (unsigned)((t / block.x) % block.y), (unsigned)(t / (block.x * block.y))};
                swapcontext(&sched, &fibers[t].ctx);
                if (!fibers[t].done) live++;
            }
            count_result = count_acc;
            count_acc = 0;
        }
    }
}
} // namespace refcpu
