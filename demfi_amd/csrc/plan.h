// What the host units of the forward context share: the context itself and the few functions that cross a unit boundary.
//   conv_build.cpp  a convolution call site -> demfi_conv descriptor + channel maps (conv_shape), -> packed weights (conv_pack)
//   layout.cpp      the workspace layout (compute_layout) and the liveness arena (plan_arena)
//   plan.cpp        the layer table and the launch plan of DeMFInet.forward (run_builder)
//   ctx.cpp         context life cycle, the C ABI entry points, the op interpreter (demfi_run_op)
#pragma once
#include "common.h"
#include <map>
#include <string>
#include <vector>

namespace plan {

struct Tensor {
    int64_t off = -1;
    int kind = 0;              // 0 fat [B,h,w,C] path dtype, 1 thin [C,h,w] fp32, 2 raw int64
    int d[4] = {0, 0, 0, 0};   // fat: B,h,w,C; thin: C,h,w,1; raw: n,1,1,1
    int64_t bytes = 0;
    int64_t cstride = 0;       // per-t buffers: bytes between the copies of consecutive per-t contexts (tensor-major layout), 0 = trunk buffer
    int id = 0;                // > 0: index into demfi_ctx::id_cstride; views built from the tensor carry it in demfi_view._pad while the plan is built
};

// Liveness plan of one buffer set (round 5, the workspace arena): the big activation buffers whose first access in the launch
// sequence is a write share ONE arena; off = byte offset of the buffer's footprint inside the arena, size = arena bytes.
struct ArenaPlan { std::map<std::string, int64_t> off; int64_t size = 0; int64_t cstride = 0; bool on = false; };     // cstride: context stride of every arena member of a per-t set (the slot size)

struct Weight { std::vector<float> data; std::vector<int64_t> shape; };

struct Layer { int cout, cin, kh, kw; };

typedef std::map<std::string, Tensor> BufSet;
typedef std::vector<demfi_op> OpList;

// A convolution call site shaped for the kernel that owns it: the descriptor (weight / bias / zero-page pointers still unset) and the
// channel maps its weights are packed by.
struct ConvShape {
    demfi_conv d;
    std::vector<int32_t> cin_map, cout_map, nks;   // packed input channel -> cin (-1: padding), packed cout -> cout, k-steps per chunk
    int64_t wbytes = 0;                            // size of the packed weights
    int64_t macs = 0;
};

// pad_y / pad_x < 0: the layer's own padding; grid_div: see the record-size choice in conv_shape
int conv_shape(int dtype, int H, int W, int stride, int batch, const Layer& l, const demfi_conv_src* srcs, int n_srcs,
               const demfi_conv_dst* dsts, int n_dsts, ConvShape& out, const char* name, int pad_y = -1, int pad_x = -1, int grid_div = 1);
// weights [cout,cin,kh,kw] / bias [cout] (may be NULL) of layer l in the order of s: wpack gets s.wbytes bytes, bias s.d.cout_pad floats
int conv_pack(const ConvShape& s, const Layer& l, const float* w, const float* bias, std::vector<uint8_t>& wpack, std::vector<float>& bias_packed);

}  // namespace plan

struct demfi_ctx {
    int H, W, N, dtype, n_trunk, n_ctx;
    int op_kind = 0, op_batch = 1;                     // 0: the DeMFI-Net forward; 1 / 2: a single-call operator context (SepConvGRU / FGAC, ABI v7)
    demfi_hparams hp;
    std::map<std::string, plan::Weight> weights;
    std::map<std::string, plan::Layer> table;
    // layout (computed at create time: offsets are relative to the workspace base)
    int64_t w_region = 0, w_bytes = 0, desc_off = 0, zero_off = 0, total = 0, n_descs = 0;
    std::vector<plan::BufSet> tr_bufs;                 // [trunk]
    std::vector<std::vector<plan::BufSet>> t_bufs;     // [trunk][c]
    std::vector<int64_t> id_cstride;                   // tensor id -> context stride in bytes (0: trunk buffer); [0] unused
    plan::ArenaPlan arena_t, arena_tr;                 // liveness plans of the per-t / trunk buffer sets (empty: every buffer has its own memory)
    // after bind
    bool bound = false, on_host = false;
    char* base = nullptr;
    std::vector<demfi_conv> descs;
    std::vector<plan::OpList> tr_ops;                  // [trunk]
    std::vector<std::vector<plan::OpList>> head_ops;   // [trunk][c]
    std::vector<std::vector<std::vector<plan::OpList>>> iter_ops;   // [trunk][c][it]
    // the same per-t segment as ONE launch sequence over all n_ctx contexts of a trunk set (demfi_forward_tb): every
    // convolution runs once with batch x n_ctx (the copies of a per-t buffer are contiguous), point-wise ops once per context
    std::vector<plan::OpList> tb_head_ops;             // [trunk]
    std::vector<std::vector<plan::OpList>> tb_iter_ops;   // [trunk][it]
    // fusion decisions of the sizing pass ("<kind>:<name>" per fused launch, in plan order).  The arena gives the buffers a fused launch
    // never touches (the scratch between the convolutions of a residual block, the z buffer of a GRU half-step) NO memory, so the
    // bind pass must fuse exactly the same launches: checked in run_builder.
    std::vector<std::string> fused_dry, fused_now;
    std::vector<uint8_t> host_blob;                    // packed weights + biases staged on the host
    std::map<std::string, std::pair<int64_t, int64_t>> pack_cache;   // layer signature -> (w_off, b_off) inside the blob
    int64_t blob_fill = 0;
};

namespace plan {

inline int esz_of(const demfi_ctx* c) { return c->dtype == DEMFI_F32 ? 4 : 2; }

void layer_table(demfi_ctx* c);                                       // plan.cpp: the reference's layers and their shapes
int run_builder(demfi_ctx* c, bool dry);                              // plan.cpp: dry = the sizing pass (no weights, nothing is written)
void compute_layout(demfi_ctx* c, int64_t w_bytes, int64_t n_descs);  // layout.cpp
ArenaPlan plan_arena(const demfi_ctx* c, const BufSet& set, int rep, const std::vector<const OpList*>& seq,
                     const std::vector<const OpList*>& foreign, const std::vector<std::string>& allow);

}  // namespace plan
