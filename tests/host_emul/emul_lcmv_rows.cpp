// The chain's launch plan (csrc/chain_plan.hpp) for an lcmv batch that emits R beams per stream (bf_config.lcmv_out_beams): emul.cpp's
// emul_chain_plan with ChainShape::lcmv_rows filled in.  Built by tests/test_lcmv_beams_cpu.py with g++; no device code.
#include <cstring>

#include "../../beamform_amd/csrc/chain_plan.hpp"

// in[23] = ChainShape's members up to gsc_serial, in order; lcmv_rows < 0: the member is left as a shape written without it has it;
// out[26] = emul_chain_plan's 25 values, then ChainPlan::rows
extern "C" void emul_chain_plan_lcmv_rows(const long *in, int lcmv_rows, long *out) {
    bf::ChainShape c{(int)in[0], (int)in[1], (int)in[2], (int)in[3], (int)in[4], (int)in[5], (int)in[6], (int)in[7], (int)in[8], in[9] != 0,
                     in[10], (int)in[11], (int)in[12], (int)in[13], (int)in[14], (int)in[15], in[16] != 0, (int)in[17], in[18] != 0,
                     in[19] != 0, in[20] != 0, (int)in[21], in[22] != 0};
    if (lcmv_rows >= 0) c.lcmv_rows = lcmv_rows;
    const bf::ChainPlan p = bf::chain_decide(c);
    const long v[26] = {p.algo, p.layout, (long)p.front, p.z48, (long)p.bins, p.mp, p.km, p.wps, (long)p.rec, p.expand, (long)p.istft, (long)p.tail,
                        p.t0, p.t1, p.t2, p.yh32, p.mpf32, p.band_rows, p.yh_lo, p.yh_hi, (long)p.z_bytes, (long)p.yh_bytes, (long)p.yraw_elems,
                        (long)p.frames_elems, p.fused(), p.rows};
    memcpy(out, v, sizeof(v));
}
