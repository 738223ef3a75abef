// cuda_host.cpp -- the block runner of the host execution layer (cuda_host.h).
//
// Blocks run one after another on the calling OS thread.  A kernel without a barrier is a loop
// over its threads.  A kernel with one gets a cooperative context per thread of the block (the
// count comes from the block's dimensions, nothing else): the scheduler resumes every live
// thread in turn until it stands at a barrier or has left the kernel; when none is left
// running, the barrier opens for all that wait.  A thread that has returned no longer counts.
#include "cuda_host.h"

#include <sys/mman.h>

#include <vector>

#if defined(__SANITIZE_ADDRESS__)
#define CUDA_HOST_ASAN 1
#elif defined(__has_feature)
#if __has_feature(address_sanitizer)
#define CUDA_HOST_ASAN 1
#endif
#endif
#ifdef CUDA_HOST_ASAN
#include <sanitizer/common_interface_defs.h>
#endif

uint3 threadIdx, blockIdx;
dim3 blockDim, gridDim;

namespace cuda_host {

Stats stats;
void reset_stats() { memset(&stats, 0, sizeof(stats)); }

// ------------------------------------------------------------------------- context switching
#if defined(__x86_64__)
// Saves the callee-saved registers on the current stack, stores the stack pointer in *from and
// continues on the stack `to` (System V AMD64).  Control words are the same in every context.
// swapcontext (the fallback below, for other architectures) would do the same job, but it
// makes a signal-mask system call per switch, and RowMatch_Kernel at 3000 x 9000 switches 54
// million times (32 threads, 283 barriers, 3000 blocks, there and back): seconds against minutes.
extern "C" void cuda_host_switch(void** from, void* to);
asm(R"(
.text
.p2align 4
.hidden cuda_host_switch
.globl cuda_host_switch
.type cuda_host_switch,@function
cuda_host_switch:
    pushq %rbp
    pushq %rbx
    pushq %r12
    pushq %r13
    pushq %r14
    pushq %r15
    movq %rsp, (%rdi)
    movq %rsi, %rsp
    popq %r15
    popq %r14
    popq %r13
    popq %r12
    popq %rbx
    popq %rbp
    ret
.size cuda_host_switch,.-cuda_host_switch
.section .note.GNU-stack,"",@progbits
.text
)");
struct Context { void* sp = nullptr; };
static void context_make(Context* c, char* stack, size_t size, void (*entry)()) {
    void** top = (void**)(((uintptr_t)stack + size) & ~(uintptr_t)15);
    top[-1] = nullptr;            // return address of entry(): never used, entry() does not return
    top[-2] = (void*)entry;       // popped by the switch's ret; rsp is then 8 mod 16, as after a call
    for (int i = 3; i <= 8; i++) top[-i] = nullptr;
    c->sp = top - 8;
}
static inline void context_switch(Context* from, Context* to) { cuda_host_switch(&from->sp, to->sp); }
#else
#include <ucontext.h>
struct Context { ucontext_t uc; };
static void context_make(Context* c, char* stack, size_t size, void (*entry)()) {
    getcontext(&c->uc);
    c->uc.uc_stack.ss_sp = stack;
    c->uc.uc_stack.ss_size = size;
    c->uc.uc_link = nullptr;
    makecontext(&c->uc, entry, 0);
}
static inline void context_switch(Context* from, Context* to) { swapcontext(&from->uc, &to->uc); }
#endif

// ---------------------------------------------------------------------------------- scheduler
constexpr size_t kStackBytes = 256 << 10;

struct Fiber {
    Context ctx;
    char* stack = nullptr;
    void* fake_stack = nullptr;   // AddressSanitizer's bookkeeping for this context
    bool done = false;
};

static std::vector<Fiber> g_fibers;
static Context g_scheduler;
static void* g_scheduler_fake = nullptr;
static const void* g_scheduler_bottom = nullptr;
static size_t g_scheduler_size = 0;
static int g_current = -1;        // fiber running now; -1 on the scheduler's stack
static const std::function<void()>* g_body = nullptr;

static inline void to_scheduler(Fiber& f) {
#ifdef CUDA_HOST_ASAN
    __sanitizer_start_switch_fiber(f.done ? nullptr : &f.fake_stack, g_scheduler_bottom, g_scheduler_size);
#endif
    context_switch(&f.ctx, &g_scheduler);
#ifdef CUDA_HOST_ASAN
    __sanitizer_finish_switch_fiber(f.fake_stack, &g_scheduler_bottom, &g_scheduler_size);
#endif
}

static void fiber_entry() {
    Fiber& f = g_fibers[g_current];
#ifdef CUDA_HOST_ASAN
    __sanitizer_finish_switch_fiber(nullptr, &g_scheduler_bottom, &g_scheduler_size);
#endif
    (*g_body)();
    f.done = true;
    to_scheduler(f);
    abort();   // a finished context is never resumed
}

void syncthreads() {
    if (g_current < 0) {
        fprintf(stderr, "cuda_host: __syncthreads() in a kernel launched without barrier support\n");
        abort();
    }
    const uint3 t = threadIdx;
    to_scheduler(g_fibers[g_current]);
    threadIdx = t;
}

static void resume(int i) {
    Fiber& f = g_fibers[i];
    g_current = i;
#ifdef CUDA_HOST_ASAN
    __sanitizer_start_switch_fiber(&g_scheduler_fake, f.stack, kStackBytes);
#endif
    context_switch(&g_scheduler, &f.ctx);
#ifdef CUDA_HOST_ASAN
    __sanitizer_finish_switch_fiber(g_scheduler_fake, nullptr, nullptr);
#endif
    g_current = -1;
}

static void run_block_with_barriers(int nthreads) {
    if ((int)g_fibers.size() < nthreads) {
        const size_t old = g_fibers.size();
        g_fibers.resize(nthreads);
        for (size_t i = old; i < g_fibers.size(); i++) {
            void* p = mmap(nullptr, kStackBytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
            if (p == MAP_FAILED) { perror("cuda_host: mmap"); abort(); }
            g_fibers[i].stack = (char*)p;
        }
    }
    for (int i = 0; i < nthreads; i++) {
        g_fibers[i].done = false;
        g_fibers[i].fake_stack = nullptr;
        context_make(&g_fibers[i].ctx, g_fibers[i].stack, kStackBytes, fiber_entry);
    }
    int live = nthreads;
    while (live > 0) {
        // One round: every live thread runs to its next barrier or to its end.
        for (int i = 0; i < nthreads; i++) {
            if (g_fibers[i].done) continue;
            threadIdx.x = (unsigned)i % blockDim.x;
            threadIdx.y = (unsigned)i / blockDim.x % blockDim.y;
            threadIdx.z = (unsigned)i / (blockDim.x * blockDim.y);
            resume(i);
            if (g_fibers[i].done) live--;
        }
    }
}

void launch_impl(dim3 grid, dim3 block, bool has_barrier, const std::function<void()>& body) {
    if (g_body) { fprintf(stderr, "cuda_host: nested launch\n"); abort(); }
    stats.launches++;
    stats.last_oob = stats.last_clamped = 0;
    gridDim = grid;
    blockDim = block;
    g_body = &body;
    const int nthreads = (int)(block.x * block.y * block.z);
    for (unsigned bz = 0; bz < grid.z; bz++)
        for (unsigned by = 0; by < grid.y; by++)
            for (unsigned bx = 0; bx < grid.x; bx++) {
                blockIdx = uint3{bx, by, bz};
                stats.blocks++;
                if (has_barrier) {
                    run_block_with_barriers(nthreads);
                    continue;
                }
                for (unsigned tz = 0; tz < block.z; tz++)
                    for (unsigned ty = 0; ty < block.y; ty++)
                        for (unsigned tx = 0; tx < block.x; tx++) {
                            threadIdx = uint3{tx, ty, tz};
                            body();
                        }
            }
    g_body = nullptr;
}

}  // namespace cuda_host

// Device memory is host memory.  Fresh allocations are filled with 0xFF bytes (a NaN as float,
// -1 as int) so that a kernel reading what no kernel wrote shows up in the results.
cudaError_t cudaMalloc(void** p, size_t bytes) {
    *p = malloc(bytes ? bytes : 1);
    if (!*p) return 2;
    memset(*p, 0xFF, bytes);
    return cudaSuccess;
}
cudaError_t cudaFree(void* p) {
    free(p);
    return cudaSuccess;
}
