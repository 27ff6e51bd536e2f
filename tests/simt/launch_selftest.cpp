// TEST INFRASTRUCTURE ONLY: csrc/common.h's mq_launch as a stand-alone host program (tests/test_simt_kernels_cpu.py compiles and runs it).
// The "kernels" are plain functions and a launch is a plain call -- no fibers, so the program can also be built with -fsanitize=thread:
//   launch_selftest            every rule of mq_launch below, one host thread
//   launch_selftest threads    two host threads, one device index each, the same kernels (the contract of common.h: one thread per GPU)
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) kernel(__VA_ARGS__)
#include "common.h"
#include <stdio.h>
#include <thread>

thread_local int simt::g_error = 0;       // (the program does not link the fiber runtime that owns it)

static void kern_a(int* ran) { ++*ran; }
static void kern_b(int* ran) { ++*ran; }
static void kern_c(int* ran) { ++*ran; }
static void kern_faulty(int* ran) { ++*ran; simt::g_error = hipErrorLaunchFailure; }

static int failures = 0;
#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) { ++failures; printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); } \
  } while (0)

template <auto K>
static int go(size_t smem, int* ran) { return mq_launch<K>(dim3(1), dim3(64), smem, nullptr, ran); }
template <auto K>
static int calls(int dev, int* bytes = nullptr) { return simt::attr_calls((const void*)K, dev, bytes); }

static void single_thread() {
  int ran = 0, bytes = 0;
  // repeated equal size: one attribute call for this kernel on this device, every launch runs
  simt::g_device = 3;
  for (int i = 0; i < 3; ++i) EXPECT(go<kern_a>(70000, &ran) == 0);
  EXPECT(ran == 3 && calls<kern_a>(3, &bytes) == 1 && bytes == 70000);
  // a smaller size: none; a larger one: a second call with that size
  EXPECT(go<kern_a>(1000, &ran) == 0 && calls<kern_a>(3) == 1);
  EXPECT(go<kern_a>(90000, &ran) == 0 && calls<kern_a>(3, &bytes) == 2 && bytes == 90000);
  EXPECT(go<kern_a>(70000, &ran) == 0 && calls<kern_a>(3) == 2);
  // another kernel, another device: their own state
  EXPECT(calls<kern_b>(3) == 0);
  EXPECT(go<kern_b>(1000, &ran) == 0 && calls<kern_b>(3, &bytes) == 1 && bytes == 1000 && calls<kern_a>(3) == 2);
  simt::g_device = 4;
  EXPECT(go<kern_a>(1000, &ran) == 0 && calls<kern_a>(4, &bytes) == 1 && bytes == 1000 && calls<kern_a>(3) == 2);
  EXPECT(go<kern_a>(1000, &ran) == 0 && calls<kern_a>(4) == 1);
  // no dynamic LDS: the attribute is never touched
  simt::g_device = 5;
  ran = 0;
  for (int i = 0; i < 3; ++i) EXPECT(go<kern_a>(0, &ran) == 0);
  EXPECT(ran == 3 && calls<kern_a>(5) == 0);
  // unknown device (index out of range, or the query fails): the attribute is set on every call
  simt::g_device = 32;
  for (int i = 0; i < 3; ++i) EXPECT(go<kern_a>(500, &ran) == 0);
  EXPECT(calls<kern_a>(32) == 3);
  simt::g_device = -1;
  for (int i = 0; i < 2; ++i) EXPECT(go<kern_a>(500, &ran) == 0);
  EXPECT(calls<kern_a>(-1) == 2);
  simt::g_device = 6;
  simt::g_device_error = 101;
  for (int i = 0; i < 2; ++i) EXPECT(go<kern_a>(500, &ran) == 0);
  EXPECT(calls<kern_a>(6) == 2);
  simt::g_device_error = 0;
  EXPECT(go<kern_a>(500, &ran) == 0 && go<kern_a>(500, &ran) == 0 && calls<kern_a>(6) == 3);      // known again: once, then remembered
  // a failing attribute call: its code, no launch, no mark -- the next call tries again
  simt::g_device = 7;
  ran = 0;
  simt::g_attr_fail_next = 98;
  EXPECT(go<kern_c>(2000, &ran) == 98 && ran == 0 && calls<kern_c>(7) == 0);
  EXPECT(go<kern_c>(2000, &ran) == 0 && ran == 1 && calls<kern_c>(7) == 1);
  EXPECT(go<kern_c>(2000, &ran) == 0 && ran == 2 && calls<kern_c>(7) == 1);
  simt::g_attr_fail_next = 98;                                                                     // ... and a failed RAISE keeps the old maximum
  EXPECT(go<kern_c>(3000, &ran) == 98 && ran == 2);
  EXPECT(go<kern_c>(3000, &ran) == 0 && ran == 3 && calls<kern_c>(7, &bytes) == 2 && bytes == 3000);
  // an error raised by the launch is returned (and consumed)
  ran = 0;
  EXPECT(go<kern_faulty>(100, &ran) == hipErrorLaunchFailure && ran == 1);
  EXPECT(go<kern_a>(0, &ran) == 0);
}

static void worker(int dev, int* ran) {
  simt::g_device = dev;
  for (int i = 0; i < 2000; ++i) {
    if (go<kern_a>(1000 + (i & 1023), ran) != 0) ++failures;    // a growing size: loads and stores of the per-device maximum all the way
    if (go<kern_b>(64, ran) != 0) ++failures;
  }
}
static void two_threads() {
  int ran[2] = {0, 0};
  std::thread t0(worker, 10, &ran[0]), t1(worker, 11, &ran[1]);
  t0.join();
  t1.join();
  EXPECT(ran[0] == 4000 && ran[1] == 4000);
  for (int dev = 10; dev < 12; ++dev) {
    int bytes = 0;
    EXPECT(calls<kern_a>(dev, &bytes) == 1024 && bytes == 1000 + 1023);
    EXPECT(calls<kern_b>(dev) == 1);
  }
}

int main(int argc, char** argv) {
  if (argc > 1 && argv[1][0] == 't') two_threads();
  else single_thread();
  printf(failures ? "FAILED: %d\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
