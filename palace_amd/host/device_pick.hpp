// Which GPU an executable works on.  The reference's stages are one process each and know nothing of devices; a node with eight
// MI355X runs eight samples side by side with PALACE_DEVICE=<k> per pipeline (the `weak` reading of "N GPUs": no collective in the
// data path).  Default: device 0.  When nothing else restricts the visible devices, the choice is made by ROCR_VISIBLE_DEVICES,
// set here BEFORE the process's first HIP call: the runtime then brings up one device instead of every device of the node (its
// start-up is most of eref's wall time), and the chosen device is ordinal 0 of the process.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <iostream>
#include <string>

#include "../../include/palace_hip.h"
#include "fast_exit.hpp"

namespace palace_host {

// call once, from main(), before any thread that may touch HIP exists; returns the ordinal to hand to palace_ctx_create
inline int pick_device()
{
    static const int chosen = [] {
        const char* d = std::getenv("PALACE_DEVICE");
        int dev = (d && *d) ? std::atoi(d) : 0;
        if (dev < 0) dev = 0;
        for (const char* k : {"ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "GPU_DEVICE_ORDINAL"})
            if (std::getenv(k)) return dev;                       // somebody has chosen the visible set: PALACE_DEVICE is an ordinal within it
        if (gpu_touched_before_main()) return dev;               // (a runtime is up already: the variable would come too late)
        ::setenv("ROCR_VISIBLE_DEVICES", std::to_string(dev).c_str(), 1);
        return 0;
    }();
    return chosen;
}

// The frame of an executable that works on one device: the context on the picked device, body(ctx) -> exit code, the context
// destroyed.  A context that cannot be made, or an exception from the body, is `<prog>: <message>` on stderr and exit code 1.
template <class Body> int with_device(const char *prog, Body body)
{
    palace_ctx *ctx = nullptr;
    if (palace_ctx_create(pick_device(), &ctx)) { std::cerr << prog << ": " << palace_last_error() << "\n"; return 1; }
    int code = 1;
    try {
        code = body(ctx);
    } catch (const std::exception &e) { std::cerr << prog << ": " << e.what() << "\n"; }
    palace_ctx_destroy(ctx);
    return code;
}

// Two frames because they leave differently: with_device returns through the teardown (the context destroyed, main's return), while
// device_tool leaves through FastExit::done, the caller going on while the teardown happens behind it (fast_exit.hpp).
// The frame of make_fa_from_path, split_fastg, readqc, make_final_fa, filter_result and faidx, called when the command line is parsed: the
// forked start, the picked device, the context, body(ctx, trace).  No device, or an exception from the body, is one `<prog>: ...` line
// on stderr behind whatever stdout holds, and exit code 1; a body that has said in words of its own why it fails (faidx, whose lines
// are samtools') throws SaidAlready: exit code 1 and no further line.  (eref, generateGraph and matching bring the context up on a thread beside
// their input and keep frames of their own.)
struct SaidAlready {};
template <class Body> int device_tool(const char *prog, Body body)
{
    FastExit fast_exit = fast_exit_begin();   // from here on this is the worker process
    const int device = pick_device();         // before anything touches HIP
    Trace tr(prog);
    palace_ctx *ctx = nullptr;
    if (palace_ctx_create(device, &ctx) != PALACE_OK) {
        std::fprintf(stderr, "%s: no GPU device to work on (%s); there is no CPU path\n", prog, palace_last_error());
        return 1;
    }
    tr.lap("device up");
    try {
        body(ctx, tr);
    } catch (const SaidAlready &) {
        std::fflush(stdout);
        return 1;
    } catch (const std::exception &e) {
        std::fflush(stdout);
        std::fprintf(stderr, "%s: %s\n", prog, e.what());
        return 1;
    }
    fast_exit.done(0);          // outputs are complete and closed: the caller goes on, the teardown happens behind it
}

}  // namespace palace_host
