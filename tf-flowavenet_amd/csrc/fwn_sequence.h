// What the two host sequencers share (api.hip: inference passes; train_api.hip: the training step): the kind of a pass, and
// the ONE statement of the ragged forward rules - which rows are filled with what, and where between the stage launches.
// DESIGN.md section 8 states the training backward as the adjoint of these fills, so training's forward half runs them through
// the walks below and cannot drift from inference.  Everything here is defined in api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fwn.h"

inline int dilation_of(int layer) {  // kernel_size ** n, modules.py:152
    int dil = 1;
    for (int i = 0; i < layer; ++i) dil *= 3;
    return dil;
}
inline int hop_of(const fwn_model_desc* m) {
    int hop = 1;
    for (int i = 0; i < m->n_up; ++i) hop *= m->up_scale[i];
    return hop;
}

// ---- the kind of a pass: every entry point and workspace query names one; pass_traits derives what it needs ----
enum PassKind {
    PASS_FORWARD,            // fwn_model_forward (and every layout query of the plain passes)
    PASS_FORWARD_DDI,        // ... with the local data-dependent init
    PASS_FORWARD_INIT,       // fwn_model_forward_init: moments -> reduce callback -> tables
    PASS_REVERSE,            // fwn_model_reverse
    PASS_REVERSE_RAGGED,     // fwn_model_reverse_ragged
    PASS_FORWARD_RAGGED,     // fwn_model_forward_ragged
    PASS_INIT_RAGGED,        // fwn_model_forward_init_ragged
    PASS_TRAIN,              // fwn_train_loss_and_grads
    PASS_TRAIN_RAGGED,       // fwn_train_loss_and_grads_ragged
    PASS_FORWARD_WINDOWS,    // fwn_model_forward_windows: the ragged forward's form on full-length windows (no lengths: no fills)
};
struct PassTraits {
    const char* what;        // the entry point's name in error messages
    bool reverse;
    int init;                // 0 none, 1 local two-pass init, 2 moments -> reduce callback (may be NULL) -> tables
    // per-clip lengths: every flow a launch per stage - no one-launch flows, no chaining (the zero-fills run between the
    // stages; the chained front conv reads out_b rows inside the launch that writes them) - plus a copy of the mel to mask
    bool ragged;
    bool logdet;             // ... forward: also one flow's Z (reused by the next flow) and every flow's per-clip log-det sums
    bool mompart;            // ... init: also the chunk sums of one flow's masked moments (reused by the next flow)
};
inline PassTraits pass_traits(PassKind k) {
    switch (k) {
    case PASS_FORWARD_DDI:    return {"fwn_model_forward", false, 1, false, false, false};
    case PASS_FORWARD_INIT:   return {"fwn_model_forward", false, 2, false, false, false};
    case PASS_REVERSE:        return {"fwn_model_reverse", true, 0, false, false, false};
    case PASS_REVERSE_RAGGED: return {"fwn_model_reverse_ragged", true, 0, true, false, false};
    case PASS_FORWARD_RAGGED: return {"fwn_model_forward_ragged", false, 0, true, true, false};
    case PASS_INIT_RAGGED:    return {"fwn_model_forward_init_ragged", false, 2, true, true, true};
    case PASS_TRAIN:          return {"fwn_train_loss_and_grads", false, 0, false, false, false};
    case PASS_TRAIN_RAGGED:   return {"fwn_train_loss_and_grads_ragged", false, 0, true, true, false};
    case PASS_FORWARD_WINDOWS: return {"fwn_model_forward_windows", false, 0, true, true, false};
    default:                  return {"fwn_model_forward", false, 0, false, false, false};
    }
}

// ---- "the rows past each clip's end" of a ragged batch: len[B] on the device (samples; clamped to the buffer by the kernels).
// Every method is a no-op for a plain batch (len NULL).
struct ClipRows {
    const int32_t* len;
    long B;
    hipStream_t st;
    // rows [len / samples_per_row, rows) of every clip of a [B][rows][row_bytes] buffer := 0
    void zero(void* base, long rows, long row_bytes, int samples_per_row) const;
    // the same for both planes [2][B][T / 2] fp32: clip b's samples sit at [b][0, len / 2) at every block (a row of block i is
    // 2^i of them, and len is a multiple of 2^n_block)
    void zero_planes(float* planes, long T) const;
    // -shift[tau] into those rows of x_a [B][rows][Ch] fp32: the front conv applies ActNorm on the fly, (v + shift) * scale, and
    // then reads exact zeros there - the padding a clip on its own gets behind ActNorm
    void neg_shift(float* xa, long rows, int Ch, const float* shift) const;
};

// ---- the up-sampling stages: mel [B][T / hop][num_mels] -> the conditioning planes.  Ragged: the stages run on a copy of the mel
// with the frames past each clip's end zeroed, and so is every inner stage's output - the transposed conv of the next stage
// reads one row across a clip's end (training's up-sampling backward reads these very buffers).  The last stage's rows past
// the end stay as they come out: the conditioning is pointwise in time.
struct UpsampleBufs {
    float* mel_copy;                       // [B][T / hop][num_mels] fp32, ragged only
    float* inner[FWN_MAX_UPSAMPLE];        // output of stage n (fp32), every stage but the last
    void* cplanes;                         // the last stage's output
    const float* const* bias_dev;          // the stages' biases on the device (training), or NULL: the model's host floats
};
// returns non-zero where the mel copy could not be enqueued
int fwn_run_upsample(const fwn_model_desc* m, long B, long T, const float* mel, const UpsampleBufs& u, const ClipRows& rows);

// ---- one flow's stages up to its last gate: [-shift fill,] front conv, zero-fill of h, then per layer the gate and - where there
// is a next layer - the res conv and the zero-fill of h.  The caller states the buffers; the walk guesses nothing.
struct FlowStages {
    void* h[FWN_MAX_LAYERS];               // h[l]: input of layer l's gate (h[0]: the front conv's output)
    void* o[FWN_MAX_LAYERS];
    void* aux[FWN_MAX_LAYERS];             // the gate's auxiliary output for the backward, NULL: not kept
    void* h8[FWN_MAX_LAYERS];              // != NULL: layer l runs the fp8 gate on this e4m3 copy of h[l], which h[l]'s producer writes
    bool gate_stream;                      // the fragment-order gate weights (fwn_flow_desc.Wgs) may be used
    void* front_scratch;                   // the front conv's scratch
    bool have_h0;                          // h[0] is already there (the previous flow's tail wrote it)
};
// ca / P: the conditioning plane (fused) or the flow's hoisted P [L][M][512] - exactly one
void fwn_run_stages(const fwn_flow_desc* d, const FlowStages& s, float* xa, const void* ca, const float* P, int M, int Ti, int inverse,
                    const ClipRows& rows);
