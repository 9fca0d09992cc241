// k_tcptrace.hip -- igx_tcp_classify: the per-row rules of trace tcp's probes (k_tcptrace.h), one
// lane per row.  Reads the raw probe columns, writes the tuple key, the row's kind for
// igx_chain_join, its own event and the thread key.  include/igx.h has the contract.
#include "k_common.h"
#include "k_tcptrace.h"

static_assert(IGX_CJ_ENTER == TCP_K_ENTER && IGX_CJ_PASS == TCP_K_PASS && IGX_CJ_ABORT == TCP_K_ABORT &&
                  IGX_CJ_TAKE == TCP_K_TAKE && IGX_CJ_DROP == TCP_K_DROP && IGX_TCP_NO_KIND == TCP_K_NONE,
              "enum igx_cj_kind and the codes of k_tcptrace.h");
static_assert(IGX_TCP_CONNECT_ENTER == TCP_P_CONNECT_ENTER && IGX_TCP_CONNECT_RETURN == TCP_P_CONNECT_RETURN &&
                  IGX_TCP_CLOSE == TCP_P_CLOSE && IGX_TCP_SET_STATE == TCP_P_SET_STATE &&
                  IGX_TCP_ACCEPT_RETURN == TCP_P_ACCEPT_RETURN,
              "enum igx_tcp_probe and the codes of k_tcptrace.h");
static_assert(IGX_TCP_TUPLE_BYTES == 4 * TCP_TUPLE_WORDS, "tuple_key_t");

namespace {

constexpr int TB = 256;

__global__ __launch_bounds__(TB) void k_tcp_classify(igx_tcp_rows in, uint64_t n, TcpFilter f,
                                                     uint32_t *__restrict__ tuple, uint8_t *__restrict__ kind,
                                                     uint8_t *__restrict__ event, uint64_t *__restrict__ key1) {
    const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    TcpRow r;
    r.probe = in.probe[i];
    r.pid = in.pid[i];
    r.uid = in.uid[i];
    r.mntns = in.mntns[i];
    r.ret = in.ret[i];
    r.state = in.state[i];
    r.family = in.family[i];
    r.netns = in.netns[i];
    const uint4 s = reinterpret_cast<const uint4 *>(in.saddr)[i], d = reinterpret_cast<const uint4 *>(in.daddr)[i];
    r.saddr[0] = s.x, r.saddr[1] = s.y, r.saddr[2] = s.z, r.saddr[3] = s.w;
    r.daddr[0] = d.x, r.daddr[1] = d.y, r.daddr[2] = d.z, r.daddr[3] = d.w;
    r.dport = in.dport[i];
    r.sport = in.sport[i];
    r.num = in.num[i];
    TcpOut o;
    tcp_classify_row(r, f, &o);
    // 40 bytes per row at an 8-byte aligned base: five 8-byte stores
    uint2 *t = reinterpret_cast<uint2 *>(tuple + i * TCP_TUPLE_WORDS);
#pragma unroll
    for (int w = 0; w < 5; ++w) t[w] = make_uint2(o.tuple[2 * w], o.tuple[2 * w + 1]);
    kind[i] = (uint8_t)o.kind;
    event[i] = (uint8_t)o.event;
    if (key1) key1[i] = in.tid[i];
}

}  // namespace

extern "C" int igx_tcp_classify(igx_ctx *ctx, const igx_tcp_rows *rows, uint64_t nrows, uint32_t filter_pid,
                                uint32_t filter_uid, const uint64_t *mntns_set, uint32_t n_mntns, uint8_t *tuple,
                                uint8_t *kind, uint8_t *event, uint64_t *key1) {
    if (!ctx) return IGX_EINVAL;
    if (nrows > 0xFFFFFFFEull) return igx_fail(ctx, IGX_EINVAL, "tcp_classify: more than 2^32 - 2 rows");
    if (n_mntns > 1024) return igx_fail(ctx, IGX_EINVAL, "tcp_classify: more than 1024 mount namespaces");
    if (nrows == 0) return IGX_OK;
    if (!rows || !tuple || !kind || !event) return igx_fail(ctx, IGX_EINVAL, "tcp_classify: null argument");
    const igx_tcp_rows &c = *rows;
    if (!c.probe || !c.tid || !c.pid || !c.uid || !c.mntns || !c.ret || !c.state || !c.family || !c.netns ||
        !c.saddr || !c.daddr || !c.dport || !c.sport || !c.num)
        return igx_fail(ctx, IGX_EINVAL, "tcp_classify: null column");
    if (((uintptr_t)c.saddr | (uintptr_t)c.daddr) & 15)
        return igx_fail(ctx, IGX_EINVAL, "tcp_classify: addresses must be 16-byte aligned");
    if (((uintptr_t)c.mntns | (uintptr_t)tuple | (uintptr_t)key1 | (uintptr_t)mntns_set) & 7)
        return igx_fail(ctx, IGX_EINVAL, "tcp_classify: mntns, tuple, key1 and the set must be 8-byte aligned");
    if (((uintptr_t)c.tid | (uintptr_t)c.pid | (uintptr_t)c.uid | (uintptr_t)c.ret | (uintptr_t)c.netns) & 3)
        return igx_fail(ctx, IGX_EINVAL, "tcp_classify: 32-bit columns must be 4-byte aligned");
    if (((uintptr_t)c.family | (uintptr_t)c.dport | (uintptr_t)c.sport | (uintptr_t)c.num) & 1)
        return igx_fail(ctx, IGX_EINVAL, "tcp_classify: 16-bit columns must be 2-byte aligned");
    TcpFilter f;
    f.pid = filter_pid;
    f.uid = filter_uid;
    f.mntns = mntns_set;
    f.n_mntns = n_mntns;
    hipLaunchKernelGGL(k_tcp_classify, dim3((unsigned)((nrows + TB - 1) / TB)), dim3(TB), 0, ctx->stream, c, nrows, f,
                       reinterpret_cast<uint32_t *>(tuple), kind, event, key1);
    IGX_HIP(ctx, hipGetLastError());
    return IGX_OK;
}
