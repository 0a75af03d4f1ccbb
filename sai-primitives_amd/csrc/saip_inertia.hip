// The resident inertia table of the simulator (arithmetic: saip_inertia.h).
//   saip_inertia_compose  fills the table from scaled links plus payloads, one lane per instance: the words of the parts come from the part
//                         tables or are drawn between two batch-uniform bound tables, and every movable body's row is composed from them
// The table is configuration: the kernel reads the model and the parts and writes the rows, nothing else, and columns cols..ld-1 are never
// written.  Its readers are the INERTIA instantiations of the integrators (saip_dynamics.hip, saip_dynamics_oct.hip).  Every store of a
// wavefront is one contiguous run of a row.
#include <hip/hip_runtime.h>

#include "saip_device.h"
#include "saip_inertia.h"

namespace saip {

__global__ void __launch_bounds__(64) saip_inertia_compose(const InertiaComposeParams P) {
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b >= P.cols) return;
	const ModelDev& md = *P.model;
	const long long bs = P.per_instance_bodies ? (long long)P.ld : 1, bc = P.per_instance_bodies ? (long long)b : 0;
	const long long ps = P.per_instance_payloads ? (long long)P.ld : 1, pc = P.per_instance_payloads ? (long long)b : 0;
	double pw[INERTIA_MAX_PAYLOADS * INERTIA_PAYLOAD_WORDS];
	for (int w = 0; w < P.n_payloads * INERTIA_PAYLOAD_WORDS; w++)
		pw[w] = P.draw ? in_draw(P.seed_lo, P.seed_hi, P.round, INERTIA_TABLE_PAYLOADS, b, w, P.payloads[w], P.payloads_hi[w]) : P.payloads[(long long)w * ps + pc];
	for (int j = 0; j < P.n; j++) {
		double bw[INERTIA_BODY_WORDS];
		for (int k = 0; k < INERTIA_BODY_WORDS; k++) {
			const int w = INERTIA_BODY_WORDS * j + k;
			bw[k] = P.draw ? in_draw(P.seed_lo, P.seed_hi, P.round, INERTIA_TABLE_BODIES, b, w, P.bodies[w], P.bodies_hi[w]) : P.bodies[(long long)w * bs + bc];
		}
		const double mdl[INERTIA_ROW_WORDS] = {md.mass[j],       md.com[j][0],     md.com[j][1],     md.com[j][2],     md.inertia[j][0],
												md.inertia[j][1], md.inertia[j][2], md.inertia[j][3], md.inertia[j][4], md.inertia[j][5]};
		in_compose_row(mdl, bw, 1, j, P.n_payloads, P.site, pw, 1, P.rows + (long long)j * INERTIA_ROW_WORDS * P.stride + (P.stride == 1 ? 0 : (long long)b), P.stride);
	}
}

hipError_t launch_inertia_compose(const InertiaComposeParams& P, hipStream_t stream) {
	hipLaunchKernelGGL(saip_inertia_compose, dim3((P.cols + 63) / 64), dim3(64), 0, stream, P);
	return hipGetLastError();
}

}  // namespace saip
