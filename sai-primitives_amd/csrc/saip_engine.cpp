// Host side of the engine behind include/saip.h: robot constants, task stacks, device arena, launches.
// C++ (the reference is a C++ library), HIP runtime only -- no PyTorch, no Eigen.
#include <hip/hip_runtime.h>

#include <cmath>
#include <utility>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/saip.h"
#include "saip_device.h"
#include "saip_cycle_plan.h"
#include "saip_state_snapshot.h"
#include "saip_sampler.h"
#include "saip_contact.h"
#include "saip_contact_patch.h"
#include "saip_clearance.h"
#include "saip_plant.h"

namespace saip {
hipError_t launch_cycle_wg(const CycleParams& P, bool tree, hipStream_t stream);
hipError_t launch_cycle_wg_list(const CycleParams& P, hipStream_t stream);
hipError_t launch_reinit(const CycleParams& P, bool tree, hipStream_t stream);
hipError_t launch_cycle_lane(const CycleParams& P, hipStream_t stream, bool* supported);
hipError_t launch_cycle_oct(const CycleParams& P, hipStream_t stream);
hipError_t launch_cycle_wave(const CycleParams& P, hipStream_t stream);
hipError_t launch_cycle_octjf(const CycleParams& P, hipStream_t stream);
hipError_t launch_pose(const CycleParams& P, int task, double* out, bool tree, hipStream_t stream);
hipError_t launch_task_diag(const CycleParams& P, int task, const double* goal, const double* desired, int gcomps, double* out, bool tree, hipStream_t stream);
hipError_t launch_model_frames(const saip::FrameQuery& Q, bool tree, hipStream_t stream);
hipError_t launch_model_dynamics(const saip::DynQuery& Q, bool tree, hipStream_t stream);
hipError_t launch_otg_joints(const OtgDev& O, int B, int ld, int mode, hipStream_t stream);
hipError_t launch_otg_cartesian(const OtgDev& O, int B, int ld, int mode, bool tree, hipStream_t stream);
hipError_t launch_otg_pair(const OtgDev& Oc, const OtgDev& Oj, int B, int ld, hipStream_t stream);
hipError_t launch_integrate_otg_pair(const SimParams& S, const OtgDev& Oc, const OtgDev& Oj, int B, int ld, hipStream_t stream);
int otg_state_fields();
hipError_t launch_integrate(const SimParams& S, bool tree, hipStream_t stream);
hipError_t launch_rollout_record(const RecordParams& P, bool tree, hipStream_t stream);
hipError_t launch_goal_schedule(const ScheduleParams& P, hipStream_t stream);
hipError_t launch_state_gather(const SnapSeg* table, const int* unit_seg, int units, int B, const int* map, int save, hipStream_t stream);
hipError_t launch_sampler_perturb(const SamplerParams& P, hipStream_t stream);
hipError_t launch_sampler_cost(const SamplerCostParams& P, hipStream_t stream);
hipError_t launch_sampler_update(const SamplerParams& P, const double* cost, double temperature, double* w, SamplerResult* res, int* best_map, hipStream_t stream);
hipError_t launch_sampler_shift(const SamplerParams& P, int n, hipStream_t stream);
hipError_t launch_contact_apply(const ContactParams& P, bool tree, hipStream_t stream);
hipError_t launch_contact_patch_apply(const ContactPatchParams& P, bool tree, hipStream_t stream);
hipError_t launch_clearance_eval(const ClearanceParams& P, bool tree, hipStream_t stream);
hipError_t launch_clearance_add_cost(int B, int ld, const double* summary, double* cost, double w_penalty, double w_collision, double d_safe, hipStream_t stream);
hipError_t launch_clearance_summary_reset(int B, int ld, double* summary, hipStream_t stream);
hipError_t launch_plant_apply(const PlantParams& P, bool tree, hipStream_t stream);
hipError_t launch_plant_randomize(const PlantRandomParams& P, hipStream_t stream);
}  // namespace saip

using saip::CycleParams;
using saip::ModelDev;
using saip::OtgDev;
using saip::SimParams;
using saip::TaskDev;

static thread_local std::string g_err;
static saip_status fail(saip_status st, const char* fmt, ...) {
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof(buf), fmt, ap);
	va_end(ap);
	g_err = buf;
	return st;
}
namespace saip {
saip_status fail_external(saip_status st, const char* fmt, ...) {  // for the other translation units of the library (saip_comm.cpp)
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof(buf), fmt, ap);
	va_end(ap);
	g_err = buf;
	return st;
}
}  // namespace saip
#define HIP_TRY(expr)                                                                                        \
	do {                                                                                                     \
		hipError_t e_ = (expr);                                                                              \
		if (e_ != hipSuccess) return fail(SAIP_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_)); \
	} while (0)

// ------------------------------------------------------------------ tiny 3x3 helpers (row-major)
static void m3_mul(const double* A, const double* B, double* C) {
	double T[9];
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < 3; j++) T[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
	memcpy(C, T, sizeof(T));
}
static void m3_vec(const double* A, const double* v, double* o) {
	double t[3];
	for (int i = 0; i < 3; i++) t[i] = A[3 * i] * v[0] + A[3 * i + 1] * v[1] + A[3 * i + 2] * v[2];
	memcpy(o, t, sizeof(t));
}
static void m3_T(const double* A, double* B) {
	double T[9];
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < 3; j++) T[3 * i + j] = A[3 * j + i];
	memcpy(B, T, sizeof(T));
}
static void m3_eye(double* A) {
	memset(A, 0, 9 * sizeof(double));
	A[0] = A[4] = A[8] = 1.0;
}
static bool m3_is_eye(const double* A) {
	for (int i = 0; i < 9; i++)
		if (A[i] != ((i % 4 == 0) ? 1.0 : 0.0)) return false;
	return true;
}
static void rpy_to_R(const double* rpy, double* R) {  // URDF fixed-axis rpy: R = Rz(yaw) Ry(pitch) Rx(roll)
	double cr = cos(rpy[0]), sr = sin(rpy[0]), cp = cos(rpy[1]), sp = sin(rpy[1]), cy = cos(rpy[2]), sy = sin(rpy[2]);
	double Rx[9] = {1, 0, 0, 0, cr, -sr, 0, sr, cr}, Ry[9] = {cp, 0, sp, 0, 1, 0, -sp, 0, cp}, Rz[9] = {cy, -sy, 0, sy, cy, 0, 0, 0, 1}, T[9];
	m3_mul(Ry, Rx, T);
	m3_mul(Rz, T, R);
}
// eigen-decomposition of a symmetric 3x3 (cyclic Jacobi); eigenvalues descending, eigenvectors in columns of V
static void sym3_eig(const double* A_in, double* lam, double* V) {
	double A[9];
	memcpy(A, A_in, sizeof(A));
	m3_eye(V);
	for (int sweep = 0; sweep < 50; sweep++) {
		double off = fabs(A[1]) + fabs(A[2]) + fabs(A[5]);
		if (off < 1e-300) break;
		for (int p = 0; p < 2; p++)
			for (int q = p + 1; q < 3; q++) {
				double apq = A[3 * p + q];
				if (fabs(apq) < 1e-300) continue;
				double theta = (A[3 * q + q] - A[3 * p + p]) / (2 * apq);
				double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1));
				double c = 1 / sqrt(t * t + 1), s = t * c;
				for (int i = 0; i < 3; i++) {
					double a = A[3 * i + p], b = A[3 * i + q];
					A[3 * i + p] = c * a - s * b;
					A[3 * i + q] = s * a + c * b;
				}
				for (int j = 0; j < 3; j++) {
					double a = A[3 * p + j], b = A[3 * q + j];
					A[3 * p + j] = c * a - s * b;
					A[3 * q + j] = s * a + c * b;
				}
				for (int i = 0; i < 3; i++) {
					double a = V[3 * i + p], b = V[3 * i + q];
					V[3 * i + p] = c * a - s * b;
					V[3 * i + q] = s * a + c * b;
				}
			}
	}
	int idx[3] = {0, 1, 2};
	for (int a = 0; a < 3; a++)
		for (int b = a + 1; b < 3; b++)
			if (A[4 * idx[b]] > A[4 * idx[a]]) std::swap(idx[a], idx[b]);
	double Vs[9];
	for (int j = 0; j < 3; j++) {
		lam[j] = A[4 * idx[j]];
		for (int i = 0; i < 3; i++) Vs[3 * i + j] = V[3 * i + idx[j]];
	}
	memcpy(V, Vs, sizeof(Vs));
}
// SaiModel::matrixRangeBasis for a 3 x cnt matrix whose columns are `dirs` (cnt vectors of 3): orthonormal basis of
// the column space with the reference's tolerance semantics (sigma_i/sigma_0 >= 1e-3; identity when rank 3).
// Returns the rank (0 = empty range); basis (3 x rank) row-major with leading dimension 3.
static int range_basis_3(const double* dirs, int cnt, double* basis) {
	double G[9] = {0};
	for (int c = 0; c < cnt; c++)
		for (int i = 0; i < 3; i++)
			for (int j = 0; j < 3; j++) G[3 * i + j] += dirs[3 * c + i] * dirs[3 * c + j];
	const double tol = 1e-3;
	memset(basis, 0, 9 * sizeof(double));
	if (cnt <= 0 || sqrt(G[0] + G[4] + G[8]) < tol) return 0;
	double lam[3], V[9];
	sym3_eig(G, lam, V);
	double s0 = sqrt(fmax(lam[0], 0.0));
	if (s0 < tol) return 0;
	int maxr = cnt < 3 ? cnt : 3, rank = maxr;
	for (int i = maxr - 1; i > 0; i--) {
		if (sqrt(fmax(lam[i], 0.0)) / s0 < tol) rank--;
		else break;
	}
	if (rank == 3) {
		m3_eye(basis);
		return 3;
	}
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < rank; j++) basis[3 * i + j] = V[3 * i + j];
	return rank;
}

// ------------------------------------------------------------------ model
struct LinkInfo {
	std::string name;
	int body;        // movable body this link is rigidly attached to (-1: attached to the fixed base)
	double R[9], p[3];  // link frame in the body frame
};
struct saip_model {
	int n = 0;
	std::vector<LinkInfo> links;
	ModelDev dev;
	double q_lower[SAIP_MAXN], q_upper[SAIP_MAXN], vel[SAIP_MAXN], effort[SAIP_MAXN];
};

// combine rigid-body inertials expressed in one frame
struct Inertial {
	double m = 0, c[3] = {0, 0, 0}, I[9] = {0};  // I about the COM
};
static void inertial_add(Inertial& a, double m2, const double* c2, const double* I2) {
	double m = a.m + m2;
	if (m <= 0) return;
	double c[3];
	for (int i = 0; i < 3; i++) c[i] = (a.m * a.c[i] + m2 * c2[i]) / m;
	double I[9] = {0};
	auto shift = [&](double mm, const double* cc, const double* II) {
		double d[3] = {cc[0] - c[0], cc[1] - c[1], cc[2] - c[2]}, dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
		for (int i = 0; i < 3; i++)
			for (int j = 0; j < 3; j++) I[3 * i + j] += II[3 * i + j] + mm * ((i == j ? dd : 0.0) - d[i] * d[j]);
	};
	shift(a.m, a.c, a.I);
	shift(m2, c2, I2);
	a.m = m;
	memcpy(a.c, c, sizeof(c));
	memcpy(a.I, I, sizeof(I));
}

static saip_status model_create(const saip_link_desc* links, const int* parent, int n_links, saip_model** out, const char* fn);
extern "C" saip_status saip_model_create_serial_chain(const saip_link_desc* links, int n_links, saip_model** out) {
	return model_create(links, nullptr, n_links, out, "saip_model_create_serial_chain");
}
extern "C" saip_status saip_model_create_tree(const saip_link_desc* links, const int* parent, int n_links, saip_model** out) {
	return model_create(links, parent, n_links, out, "saip_model_create_tree");
}
// fn: the entry point called, for the messages
static saip_status model_create(const saip_link_desc* links, const int* parent, int n_links, saip_model** out, const char* fn) {
	if (!links || !out || n_links <= 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null or empty link list", fn);
	if (parent)
		for (int l = 0; l < n_links; l++)
			if (parent[l] < -1 || parent[l] >= l)
				return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: link %.*s has parent index %d (a parent must be -1, the fixed base, or a link "
						   "listed before it)", fn, SAIP_NAME_LEN, links[l].name, parent[l]);
	auto* M = new saip_model();
	memset(&M->dev, 0, sizeof(ModelDev));
	std::vector<Inertial> inertials;
	std::vector<int> body_parent;  // movable parent body of each movable body (-1: the base)
	for (int l = 0; l < n_links; l++) {
		const saip_link_desc& L = links[l];
		// fixed transform between the parent link's movable body frame (or the base) and this link: the parent link's own (body, R, p)
		const int pl_idx = parent ? parent[l] : l - 1;
		double Rp[9], pp[3] = {0, 0, 0};
		int body = -1;
		if (pl_idx >= 0) {
			const LinkInfo& P = M->links[pl_idx];
			body = P.body;
			memcpy(Rp, P.R, sizeof(Rp));
			memcpy(pp, P.p, sizeof(pp));
		} else {
			m3_eye(Rp);
		}
		double R0[9], Rl[9], pl[3], t[3];
		rpy_to_R(L.origin_rpy, R0);
		m3_vec(Rp, L.origin_xyz, t);
		for (int i = 0; i < 3; i++) pl[i] = pp[i] + t[i];
		m3_mul(Rp, R0, Rl);  // link frame (at q = 0) in the frame of the last movable body
		double Il[9] = {L.inertia[0], L.inertia[3], L.inertia[4], L.inertia[3], L.inertia[1], L.inertia[5], L.inertia[4], L.inertia[5], L.inertia[2]};
		if (L.joint_type == SAIP_JOINT_FIXED) {
			if (body >= 0) {  // merge the inertial into the parent movable body (links welded to the base carry no dynamics)
				double c2[3], T[9], I2[9], RlT[9];
				m3_vec(Rl, L.com, c2);
				for (int i = 0; i < 3; i++) c2[i] += pl[i];
				m3_mul(Rl, Il, T);
				m3_T(Rl, RlT);
				m3_mul(T, RlT, I2);
				inertial_add(inertials[body], L.mass, c2, I2);
			}
			memcpy(Rp, Rl, sizeof(Rl));
			memcpy(pp, pl, sizeof(pl));
		} else if (L.joint_type == SAIP_JOINT_REVOLUTE || L.joint_type == SAIP_JOINT_PRISMATIC) {
			if (M->n >= SAIP_MAXN) {
				delete M;
				return fail(SAIP_ERR_UNSUPPORTED, "robot has more than %d degrees of freedom", SAIP_MAXN);
			}
			double an = sqrt(L.axis[0] * L.axis[0] + L.axis[1] * L.axis[1] + L.axis[2] * L.axis[2]);
			if (an < 1e-12) {
				delete M;
				return fail(SAIP_ERR_INVALID_ARGUMENT, "joint of link %s has a zero axis", L.name);
			}
			int j = M->n++;
			body_parent.push_back(body);
			body = j;
			M->dev.jtype[j] = L.joint_type;
			memcpy(M->dev.R0[j], Rl, sizeof(Rl));
			memcpy(M->dev.p0[j], pl, sizeof(pl));
			for (int i = 0; i < 3; i++) M->dev.axis[j][i] = L.axis[i] / an;
			M->dev.axis_is_z[j] = (M->dev.axis[j][0] == 0.0 && M->dev.axis[j][1] == 0.0 && M->dev.axis[j][2] == 1.0) ? 1 : 0;
			Inertial in;
			inertial_add(in, L.mass, L.com, Il);
			if (L.mass <= 0) memcpy(in.c, L.com, sizeof(in.c));
			inertials.push_back(in);
			M->q_lower[j] = L.q_lower;
			M->q_upper[j] = L.q_upper;
			M->vel[j] = L.velocity_limit;
			M->effort[j] = L.effort_limit;
			M->dev.effort[j] = L.effort_limit;
			M->dev.q_lower[j] = L.q_lower;
			M->dev.q_upper[j] = L.q_upper;
			M->dev.vel_limit[j] = L.velocity_limit;
			m3_eye(Rp);
			pp[0] = pp[1] = pp[2] = 0;
		} else {
			delete M;
			return fail(SAIP_ERR_INVALID_ARGUMENT, "link %s: unknown joint type %d", L.name, L.joint_type);
		}
		LinkInfo li;
		li.name = std::string(L.name, strnlen(L.name, SAIP_NAME_LEN));
		li.body = body;
		memcpy(li.R, Rp, sizeof(Rp));
		memcpy(li.p, pp, sizeof(pp));
		M->links.push_back(li);
	}
	if (M->n == 0) {
		delete M;
		return fail(SAIP_ERR_INVALID_ARGUMENT, "robot has no movable joint");
	}
	M->dev.n = M->n;
	for (int j = 0; j < M->n; j++) {
		const Inertial& in = inertials[j];
		M->dev.mass[j] = in.m;
		memcpy(M->dev.com[j], in.c, sizeof(in.c));
		M->dev.inertia[j][0] = in.I[0];
		M->dev.inertia[j][1] = in.I[4];
		M->dev.inertia[j][2] = in.I[8];
		M->dev.inertia[j][3] = in.I[1];
		M->dev.inertia[j][4] = in.I[2];
		M->dev.inertia[j][5] = in.I[5];
		M->dev.iso_inertia[j] = (in.I[0] == in.I[4] && in.I[0] == in.I[8] && in.I[1] == 0.0 && in.I[2] == 0.0 && in.I[5] == 0.0) ? 1 : 0;
	}
	M->dev.gravity[0] = 0;
	M->dev.gravity[1] = 0;
	M->dev.gravity[2] = -9.81;
	for (int j = 0; j < M->n; j++) {  // packed per-joint records
		saip::JointRec& r = M->dev.jrec[j];
		memcpy(r.R0, M->dev.R0[j], sizeof(r.R0));
		memcpy(r.p0, M->dev.p0[j], sizeof(r.p0));
		memcpy(r.axis, M->dev.axis[j], sizeof(r.axis));
		memcpy(r.com, M->dev.com[j], sizeof(r.com));
		memcpy(r.inertia, M->dev.inertia[j], sizeof(r.inertia));
		r.mass = M->dev.mass[j];
		r.jtype = M->dev.jtype[j];
		r.axis_is_z = M->dev.axis_is_z[j];
		r.iso_inertia = M->dev.iso_inertia[j];
	}
	M->dev.all_axis_z = 1;
	for (int j = 0; j < M->n; j++)
		if (!M->dev.axis_is_z[j]) M->dev.all_axis_z = 0;
	// topology of the movable bodies: a chain after merging (every body's parent is the body before it) keeps is_tree = 0 and the serial kernels
	M->dev.is_tree = 0;
	for (int j = 0; j < M->n; j++) {
		const int pa = body_parent[j];
		M->dev.parent[j] = pa;
		if (pa != j - 1) M->dev.is_tree = 1;
		M->dev.anc[j] = (pa >= 0 ? M->dev.anc[pa] : 0u) | (1u << j);
		M->dev.desc[j] = 1u << j;
	}
	for (int j = M->n - 1; j >= 0; j--)
		if (M->dev.parent[j] >= 0) M->dev.desc[M->dev.parent[j]] |= M->dev.desc[j];
	for (int r = 0; r < 5; r++)
		for (int j = 0; j < SAIP_MAXN; j++) {
			if (j >= M->n) M->dev.jump[r][j] = -1;
			else if (r == 0) M->dev.jump[0][j] = M->dev.parent[j];
			else M->dev.jump[r][j] = M->dev.jump[r - 1][j] < 0 ? -1 : M->dev.jump[r - 1][M->dev.jump[r - 1][j]];
		}
	*out = M;
	return SAIP_OK;
}
extern "C" int saip_model_joint_parent(const saip_model* m, int joint) {
	if (!m || joint < 0 || joint >= m->n) return -2;
	return m->dev.parent[joint];
}
extern "C" void saip_model_destroy(saip_model* m) { delete m; }
extern "C" int saip_model_dof(const saip_model* m) { return m ? m->n : 0; }
extern "C" int saip_model_link_index(const saip_model* m, const char* name) {
	if (!m || !name) return -1;
	for (size_t i = 0; i < m->links.size(); i++)
		if (m->links[i].name == name) return (int)i;
	return -1;
}
extern "C" saip_status saip_model_joint_limits(const saip_model* m, double* lo, double* hi, double* vel, double* eff) {
	if (!m) return fail(SAIP_ERR_INVALID_ARGUMENT, "null model");
	for (int j = 0; j < m->n; j++) {
		if (lo) lo[j] = m->q_lower[j];
		if (hi) hi[j] = m->q_upper[j];
		if (vel) vel[j] = m->vel[j];
		if (eff) eff[j] = m->effort[j];
	}
	return SAIP_OK;
}

// ------------------------------------------------------------------ batch
struct TaskHost {
	std::string name;
	TaskDev dev;
	double P[36];
	bool otg_enabled = true;  // reference default (MotionForceTask.h:67, JointTask.h:38)
	// internal OTG of a joint task (saip_otg.hip): acceleration-limited, defaults JointTask.h:39-41
	bool otg_alloc = false, otg_inited = false, otg_limits_dirty = true;
	OtgDev otg;
	double otg_limits[3 * SAIP_MAXN];  // max velocity, max acceleration, max jerk per task dof (the jerk row only in jerk-limited mode)
	double* otg_limits_dev = nullptr;
	double* desired_dev = nullptr;
	bool vel_sat = false;
	bool full_joint = false;
	double* goal_dev = nullptr;
	double* integ_dev = nullptr;
	double* integ_new_dev = nullptr;
	double* diag_dev = nullptr;
	int integ_rows = 0;
	// per-task entry points (TemplateTask::updateTaskModel(N_prec) / computeTorques): the N_prec the task was last updated with, its
	// nullspaces N and N N_prec, its own torques and status; allocated on first use
	double *nprec_dev = nullptr, *ntask_dev = nullptr, *ntot_dev = nullptr, *ttau_dev = nullptr, *tprec_dev = nullptr;
	uint8_t* tstatus_dev = nullptr;
	bool nprec_identity = true;
	long model_epoch = -1;  // state epoch of the last updateTaskModel (-1: never)
	int sh_cycle = 0;       // how many times this task's model has been updated (CycleParams::task_cycle; ShState::last_cycle)
};
struct saip_snapshot;
static void snapshot_release_device(saip_snapshot* s);
struct saip_batch {
	const saip_model* model = nullptr;
	int B = 0, ld = 0, device = -1;
	bool finalized = false, models_valid = false, config_dirty = true, state_pushed = false;
	bool gravity_comp = false, torque_sat = false, integ_always = false, jla = false;
	KernelChoice kernel_choice = KernelChoice::Auto;
	std::string kernel_name = "none";
	std::vector<TaskHost> tasks;
	hipStream_t stream = nullptr;
	double *q = nullptr, *dq = nullptr, *tau = nullptr, *tau_bound = nullptr;
	uint8_t* status = nullptr;
	ModelDev* model_dev = nullptr;
	TaskDev* tasks_dev = nullptr;
	std::vector<void*> allocs;
	double* pose_dev = nullptr;              // [12][ld] scratch of saip_batch_get_current_pose_host
	double* task_diag_dev = nullptr;         // [24][ld] scratch of saip_batch_get_task_diagnostics_host
	bool model_only = false;                 // saip_batch_finalize_model_only: no tasks, state and model queries only
	double base_R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, base_p[3] = {0, 0, 0};  // saip_batch_set_robot_base (T_world_robot)
	double* query_dev = nullptr;             // scratch of the _host model queries, query_rows x ld
	size_t query_rows = 0;
	long state_epoch = 0;                    // bumped whenever the resident state changes (per-task models become stale)
	double* diag_tau = nullptr;              // scratch torques / status of diagnostic launches (the last cycle's results stay intact)
	uint8_t* diag_status = nullptr;
	hipEvent_t sync_event = nullptr;         // saip_batch_wait_for
	hipEvent_t time_ev[2] = {nullptr, nullptr};  // saip_batch_time_steps (created once: event creation is not part of a timed region)
	bool flag_nan = false;                   // saip_batch_set_flagged_torque_policy
	bool flagged_on_list = false;            // saip_batch_set_flagged_recompute: eight-lane kernels hand flagged instances to the list launch instead of their slow tail
	FlagList flags;                          // the device-side work list of the slow path
	bool otg_prelaunched = false;            // rollouts: the paired OTG step of the coming cycle already ran, fused with the previous integrate
	// saip_batch_rollout_recorder_attach: the observer of the rollout periods (saip_rollout_record.hip).  Its arrays are its own (freed by
	// _detach), not part of `allocs`.
	struct Recorder {
		bool attached = false;
		int capacity = 0, stride = 1, task = -1, rows = 0;
		unsigned channels = 0;
		long long period = 0;                // recorded periods so far: the global period counter p
		double* log = nullptr;               // [capacity][rows][ld], a ring over the samples (nullptr: empty channel mask)
		uint8_t* status_log = nullptr;       // [capacity][ld]
		double* summary = nullptr;           // [8][ld] (nullptr: summaries off)
	} rec;
	// saip_batch_goal_schedule_attach: time-varying goals of the rollout periods (saip_goal_schedule.hip), at most one per task.  The
	// keyframes are the schedule's own allocation (freed by _detach), not part of `allocs`.
	struct Schedule {
		bool attached = false;
		int first = 0, count = 0, K = 0, stride = 1, mode = 0, per_instance = 0, rot = 0;
		double* key = nullptr;               // [K][count][ld] (per instance) or [K][count] (batch-uniform)
	};
	std::vector<Schedule> sched;             // one slot per task once a schedule has been attached
	int n_sched = 0;                         // attached schedules
	long long sched_period = 0;              // rollout periods since the last attach / rewind: the counter c every schedule shares
	std::vector<saip_snapshot*> snapshots;   // saip_batch_snapshot_create: the live snapshots of this batch (their device memory goes with the batch)
	// saip_batch_sampler_attach: the resident rollout sampler (saip_sampler.hip), at most one per scheduled task.  It rewrites the task's
	// resident keyframes in place around a nominal plan; cost, weights, result and best map are the batch's, allocated by the first
	// attach and freed by the last detach.
	struct Sampler {
		bool attached = false;
		int d = 0, rot = 0, r_rot = 0, exempt = 0;
		double* nominal = nullptr;           // device: [K][count] the nominal plan, then [d] sigma
	};
	std::vector<Sampler> samp;               // one slot per task once a sampler has been attached
	int n_samp = 0;
	unsigned long long samp_seed = 0;
	long long samp_round = 0;
	double* samp_cost = nullptr;             // [ld]
	double* samp_w = nullptr;                // [ld] softmin weights of the last update
	int* samp_best_map = nullptr;            // [ld]
	saip::SamplerResult* samp_result = nullptr;
	// saip_batch_contact_attach: contact planes and the simulated force sensor of the resident simulator (saip_contact.hip), at most one
	// per batch.  Its arrays are configuration, scratch and readout: its own (freed by _detach), not part of `allocs` or of a snapshot.
	struct Contact {
		bool attached = false;
		int task = -1, n_planes = 0, per_instance = 0, sensor = 0;
		double rc[3] = {0, 0, 0};
		double* planes = nullptr;            // [P][8] (batch-uniform) or [P][8][ld]
		double* tau_sim = nullptr;           // [n][ld] commanded + contact torques of the substep being integrated
		double* readout = nullptr;           // [8][ld]
		double* summary = nullptr;           // [4][ld]
	} contact;
	// saip_batch_contact_patch_attach: contact patches (saip_contact_patch.hip), at most saip::PATCH_MAX per batch, on different motion-force
	// tasks, in the order they were attached (a detach closes the gap).  Never together with `contact`.  Their arrays are their own, like
	// those of `contact`; tau_sim is shared by the patches.
	struct ContactPatch {
		int task = -1, n_points = 0, n_planes = 0, per_instance = 0, sensor = 0;
		double r[saip::PATCH_MAX_POINTS][3] = {};
		double* planes = nullptr;            // [P][8] (batch-uniform) or [P][8][ld]
		double* readout = nullptr;           // [20][ld]
		double* summary = nullptr;           // [6][ld]
	} patch[saip::PATCH_MAX];
	int n_patch = 0;
	double* patch_tau_sim = nullptr;         // [n][ld], while n_patch > 0
	// saip_batch_clearance_attach: link spheres against obstacles and each other (saip_clearance.hip), at most one per batch.  Its arrays
	// are configuration, scratch and readout: its own (freed by _detach), not part of `allocs` or of a snapshot.
	struct Clearance {
		bool attached = false;
		int per_instance = 0, keep_centres = 0;
		double margin = 0;
		long long period = 0;                // monitored periods since the last _summary_reset
		saip::ClearanceGeom geom;            // the host copy of *geom_dev (zeroed by _attach)
		saip::ClearanceGeom* geom_dev = nullptr;
		double* obst = nullptr;              // [O][8] (batch-uniform) or [O][8][ld]
		double* readout = nullptr;           // [8][ld]
		double* summary = nullptr;           // [4][ld]
		double* centres = nullptr;           // [3 S][ld], keep_centres only
	} clearance;
	// saip_batch_plant_attach: the plant model of the resident simulator (saip_plant.hip), at most one per batch: actuator limits, friction,
	// joint stops and external wrenches in front of every integration substep.  Nothing in it is state: its arrays are configuration,
	// scratch and summaries, its own (freed by _detach), not part of `allocs` or of a snapshot; `period` is a host-side counter.
	struct Plant {
		bool attached = false;
		int per_instance_joints = 0, n_wrenches = 0, per_instance_wrenches = 0;
		long long period = 0;                // the period the next integration belongs to (wrench windows)
		saip::PlantSite site[saip::PLANT_MAX_WRENCHES] = {};
		double* joints = nullptr;            // [n][10] (batch-uniform) or [n][10][ld]
		double* wrenches = nullptr;          // [W][8] or [W][8][ld] (nullptr: no wrench)
		double* tau_act = nullptr;           // [n][ld] what the actuators, friction, stops and wrenches make of the commanded torques
		double* summary = nullptr;           // [4][ld]
		double* bounds = nullptr;            // joint lo [n][10], joint hi, wrench lo [W][8], wrench hi of saip_batch_plant_randomize (per-instance tables only)
	} plant;
};

static bool has_device(const saip_batch* b) { return b->device >= 0; }
static saip_status need_ready(saip_batch* b, const char* fn);

extern "C" int saip_device_count(void) {
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

extern "C" saip_status saip_batch_create(const saip_model* model, int batch_size, int device, saip_batch** out) {
	if (!model || !out) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_create: null argument");
	if (batch_size <= 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_create: batch size must be positive");
	if (device >= 0) {
		int cnt = saip_device_count();
		if (cnt <= 0) return fail(SAIP_ERR_NO_DEVICE, "no HIP device available: the engine has no CPU path");
		if (device >= cnt) return fail(SAIP_ERR_INVALID_ARGUMENT, "device %d out of range (%d devices)", device, cnt);
	}
	auto* b = new saip_batch();
	b->model = model;
	b->B = batch_size;
	b->ld = (batch_size + 31) / 32 * 32;
	b->device = device;  // < 0: configuration-only batch (host logic can be exercised; every compute call fails)
	*out = b;
	return SAIP_OK;
}
// leading dimension of the device arrays (default: B rounded up to 32).  Shards of a sharded run that differ by an instance all take the
// ld of the largest one, so that the final all-gather moves slabs of one shape (sharding.shard_ld)
extern "C" saip_status saip_batch_set_leading_dimension(saip_batch* b, int ld) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "null batch");
	if (b->finalized) return fail(SAIP_ERR_ORDER, "the leading dimension is fixed by saip_batch_finalize");
	if (ld < b->B || ld % 32 != 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "leading dimension %d: must be a multiple of 32 and at least the batch size %d", ld, b->B);
	b->ld = ld;
	return SAIP_OK;
}
extern "C" void saip_batch_destroy(saip_batch* b) {
	if (!b) return;
	if (has_device(b)) {
		(void)hipSetDevice(b->device);
		if (b->stream) (void)hipStreamSynchronize(b->stream);  // nothing of this batch may still be in flight
		if (b->sync_event) (void)hipEventDestroy(b->sync_event);
		for (hipEvent_t e : b->time_ev)
			if (e) (void)hipEventDestroy(e);
		for (void* p : b->allocs) (void)hipFree(p);
		for (void* p : {(void*)b->rec.log, (void*)b->rec.status_log, (void*)b->rec.summary})
			if (p) (void)hipFree(p);
		for (auto& S : b->sched)
			if (S.key) (void)hipFree(S.key);
		for (saip_snapshot* s : b->snapshots) snapshot_release_device(s);  // the handles stay valid for saip_snapshot_destroy
		for (auto& S : b->samp)
			if (S.nominal) (void)hipFree(S.nominal);
		for (void* p : {(void*)b->samp_cost, (void*)b->samp_w, (void*)b->samp_best_map, (void*)b->samp_result})
			if (p) (void)hipFree(p);
		for (void* p : {(void*)b->contact.planes, (void*)b->contact.tau_sim, (void*)b->contact.readout, (void*)b->contact.summary})
			if (p) (void)hipFree(p);
		for (const auto& C : b->patch)
			for (void* p : {(void*)C.planes, (void*)C.readout, (void*)C.summary})
				if (p) (void)hipFree(p);
		if (b->patch_tau_sim) (void)hipFree(b->patch_tau_sim);
		for (void* p : {(void*)b->clearance.geom_dev, (void*)b->clearance.obst, (void*)b->clearance.readout, (void*)b->clearance.summary, (void*)b->clearance.centres})
			if (p) (void)hipFree(p);
		for (void* p : {(void*)b->plant.joints, (void*)b->plant.wrenches, (void*)b->plant.tau_act, (void*)b->plant.summary, (void*)b->plant.bounds})
			if (p) (void)hipFree(p);
		if (b->stream) (void)hipStreamDestroy(b->stream);
	}
	delete b;
}
extern "C" int saip_batch_size(const saip_batch* b) { return b ? b->B : 0; }
extern "C" int saip_batch_ld(const saip_batch* b) { return b ? b->ld : 0; }
extern "C" int saip_batch_dof(const saip_batch* b) { return (b && b->model) ? b->model->n : 0; }

static saip_status check_batch(const saip_batch* b, int task, const char* fn) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null batch", fn);
	if (b->model_only) return fail(SAIP_ERR_ORDER, "%s: the batch was finalized for model queries only (no tasks)", fn);
	if (task >= (int)b->tasks.size() || task < -1) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, task);
	return SAIP_OK;
}
static void refresh_has_ki(TaskDev& d);
static void task_defaults(TaskDev& d, double dt) {
	memset(&d, 0, sizeof(TaskDev));
	d.dt = dt;
	d.decoupling = SAIP_BOUNDED_INERTIA_ESTIMATES;  // MotionForceTask.h:41-43, JointTask.h:35-37
	d.bie_threshold = 0.1;
}

extern "C" saip_status saip_batch_add_motion_force_task(saip_batch* b, const char* task_name, const char* link_name,
														const double pos_in_link[3], const double rot_in_link[9],
														const double* dirs_trans, int n_trans, const double* dirs_rot, int n_rot,
														double loop_timestep, int* task_id) {
	if (!b || !task_name || !link_name || !pos_in_link) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_add_motion_force_task: null argument");
	if (b->finalized) return fail(SAIP_ERR_ORDER, "tasks cannot be added after saip_batch_finalize");
	if ((int)b->tasks.size() >= SAIP_MAX_TASKS) return fail(SAIP_ERR_UNSUPPORTED, "more than %d tasks", SAIP_MAX_TASKS);
	int li = saip_model_link_index(b->model, link_name);
	if (li < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "link %s does not exist in the robot model", link_name);
	const LinkInfo& L = b->model->links[li];
	if (L.body < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "link %s is welded to the base: no controllable degree of freedom", link_name);
	TaskHost T;
	T.name = task_name;
	task_defaults(T.dev, loop_timestep);
	T.dev.type = saip::TASK_MOTION_FORCE;
	T.dev.body = L.body;
	double I3[9];
	m3_eye(I3);
	const double* Rin = rot_in_link ? rot_in_link : I3;
	double t[3];
	m3_vec(L.R, pos_in_link, t);
	for (int i = 0; i < 3; i++) T.dev.pos[i] = L.p[i] + t[i];
	m3_mul(L.R, Rin, T.dev.rot);
	double bt[9], br[9];
	int pr, orr;
	if (n_trans < 0 && n_rot < 0) {  // full task, MotionForceTask.cpp:28
		m3_eye(bt);
		m3_eye(br);
		pr = orr = 3;
	} else {
		if (n_trans <= 0 && n_rot <= 0)  // MotionForceTask.cpp:47-53
			return fail(SAIP_ERR_INVALID_ARGUMENT, "controlled_directions_translation and controlled_directions_rotation cannot both be empty in MotionForceTask::MotionForceTask");
		if ((n_trans > 0 && !dirs_trans) || (n_rot > 0 && !dirs_rot)) return fail(SAIP_ERR_INVALID_ARGUMENT, "null direction array");
		pr = range_basis_3(dirs_trans, n_trans > 0 ? n_trans : 0, bt);   // :55-87
		orr = range_basis_3(dirs_rot, n_rot > 0 ? n_rot : 0, br);
	}
	if (pr + orr == 0)  // :154-160
		return fail(SAIP_ERR_INVALID_ARGUMENT, "controlled_directions_translation and controlled_directions_rotation cannot both be empty in MotionForceTask::MotionForceTask");
	if (pr + orr == 1)
		return fail(SAIP_ERR_UNSUPPORTED, "rank-1 MotionForceTask: the reference's SingularityHandler never initialises its model for task_rank == 1 (SingularityHandler.cpp:100), refusing");
	memset(T.P, 0, sizeof(T.P));
	memset(T.dev.Bm, 0, sizeof(T.dev.Bm));
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < 3; j++) {
			double sp = 0, so = 0;
			for (int c = 0; c < pr; c++) sp += bt[3 * i + c] * bt[3 * j + c];
			for (int c = 0; c < orr; c++) so += br[3 * i + c] * br[3 * j + c];
			T.P[6 * i + j] = sp;
			T.P[6 * (3 + i) + 3 + j] = so;
			T.dev.Ppos[3 * i + j] = sp;
			T.dev.Pori[3 * i + j] = so;
		}
	for (int i = 0; i < 3; i++) {
		for (int c = 0; c < pr; c++) T.dev.Bm[6 * i + c] = bt[3 * i + c];
		for (int c = 0; c < orr; c++) T.dev.Bm[6 * (3 + i) + pr + c] = br[3 * i + c];
	}
	// sigmaPosition = Ppos (I - sigmaForce) Ppos^T with force space dimension 0 (MotionForceTask.cpp:927-930), same for orientation
	double PT[9];
	m3_T(T.dev.Ppos, PT);
	m3_mul(T.dev.Ppos, PT, T.dev.sig_p);
	m3_T(T.dev.Pori, PT);
	m3_mul(T.dev.Pori, PT, T.dev.sig_o);
	T.dev.k = pr + orr;
	T.dev.goal_comps = 36;  // x3 R9 v3 w3 a3 alpha3 + goal force 3 + goal moment 3 + sensed force 3 + sensed moment 3 (sensor frame)
	T.dev.kv_force = 10.0;   // MotionForceTask.h:51,54
	T.dev.kv_moment = 10.0;
	T.dev.lin_sat = 0.3;     // :63-64
	T.dev.ang_sat = M_PI / 3;
	T.dev.force_axis[2] = T.dev.moment_axis[2] = 1.0;
	T.dev.bm_identity = (pr == 3 && orr == 3) ? 1 : 0;
	T.dev.cert_kroot = pow((double)T.dev.k, -1.0 / 8.0);
	for (int i = 0; i < 3; i++) {  // MotionForceTask.h:44-49
		T.dev.kp_pos[i] = 100.0; T.dev.kv_pos[i] = 20.0; T.dev.ki_pos[i] = 0.0;
		T.dev.kp_ori[i] = 200.0; T.dev.kv_ori[i] = 28.3; T.dev.ki_ori[i] = 0.0;
	}
	T.dev.s_min = 6e-3;   // MotionForceTask.cpp:197
	T.dev.s_max = 6e-2;
	T.dev.s_abs_tol = 1e-3;  // SingularityHandler.cpp:11
	T.dev.sing_handling = 1; // _enforce_handling_strategy = true, SingularityHandler.cpp:61
	T.dev.sing_strategies = 1;  // the reference always runs its blended type-1 / type-2 strategies while the handling is enforced (:100-121, 146-158, 310-367)
	T.dev.sh_kp1 = 50.0;     // KP_TYPE_1, KV_TYPE_1, KV_TYPE_2, SingularityHandler.cpp:17-19
	T.dev.sh_kv1 = 14.0;
	T.dev.sh_kv2 = 5.0;
	T.integ_rows = 12;  // position 3, orientation 3, force 3, moment 3
	T.dev.kp_force = T.dev.kp_moment = 0.7;  // MotionForceTask.h:50-59
	T.dev.ki_force = T.dev.ki_moment = 1.3;
	T.dev.kff_force = T.dev.kff_moment = 0.95;
	T.dev.max_force_fb = 20.0;
	T.dev.max_moment_fb = 10.0;
	T.dev.Rcs[0] = T.dev.Rcs[4] = T.dev.Rcs[8] = 1.0;  // _T_control_to_sensor = identity, MotionForceTask.cpp:94
	refresh_has_ki(T.dev);
	memset(&T.otg, 0, sizeof(T.otg));
	T.otg.m = 6;
	T.otg.gs = 8;
	for (int i = 0; i < SAIP_MAXN; i++) T.otg_limits[i] = T.otg_limits[SAIP_MAXN + i] = T.otg_limits[2 * SAIP_MAXN + i] = 1.0;
	for (int i = 0; i < 3; i++) {  // MotionForceTask.h:68-71
		T.otg_limits[i] = 0.3;
		T.otg_limits[SAIP_MAXN + i] = 2.0;
		T.otg_limits[3 + i] = M_PI / 3.0;
		T.otg_limits[SAIP_MAXN + 3 + i] = 2.0 * M_PI;
	}
	b->tasks.push_back(T);
	b->config_dirty = true;
	if (task_id) *task_id = (int)b->tasks.size() - 1;
	return SAIP_OK;
}

extern "C" saip_status saip_batch_add_joint_task(saip_batch* b, const char* task_name, const double* S, int rows, double loop_timestep, int* task_id) {
	if (!b || !task_name) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_add_joint_task: null argument");
	if (b->finalized) return fail(SAIP_ERR_ORDER, "tasks cannot be added after saip_batch_finalize");
	if ((int)b->tasks.size() >= SAIP_MAX_TASKS) return fail(SAIP_ERR_UNSUPPORTED, "more than %d tasks", SAIP_MAX_TASKS);
	const int n = b->model->n;
	TaskHost T;
	T.name = task_name;
	task_defaults(T.dev, loop_timestep);
	T.dev.type = saip::TASK_JOINT;
	if (rows <= 0 || !S) {  // JointTask.cpp:18-19
		T.dev.m = n;
		T.dev.s_identity = 1;
		for (int i = 0; i < n; i++) T.dev.S[i * n + i] = 1.0;
		T.full_joint = true;
	} else {
		if (rows > n)  // a rows x n matrix with rows > n cannot have full row rank (JointTask.cpp:34-39)
			return fail(SAIP_ERR_INVALID_ARGUMENT, "joint selection matrix is not full rank in JointTask constructor");
		// full row rank check (the reference uses FullPivLU, JointTask.cpp:34-39): Gaussian elimination with full pivoting
		std::vector<double> A(S, S + (size_t)rows * n);
		double amax = 0;
		for (double v : A) amax = fmax(amax, fabs(v));
		int rank = 0;
		std::vector<char> rused(rows, 0), cused(n, 0);
		for (int step = 0; step < rows; step++) {
			int pi = -1, pj = -1;
			double best = 0;
			for (int i = 0; i < rows; i++)
				if (!rused[i])
					for (int j = 0; j < n; j++)
						if (!cused[j] && fabs(A[(size_t)i * n + j]) > best) {
							best = fabs(A[(size_t)i * n + j]);
							pi = i;
							pj = j;
						}
			if (pi < 0 || best <= amax * 1e-12 * (rows > n ? rows : n)) break;
			rank++;
			rused[pi] = cused[pj] = 1;
			for (int i = 0; i < rows; i++)
				if (!rused[i]) {
					double f = A[(size_t)i * n + pj] / A[(size_t)pi * n + pj];
					for (int j = 0; j < n; j++) A[(size_t)i * n + j] -= f * A[(size_t)pi * n + j];
				}
		}
		if (rank != rows) return fail(SAIP_ERR_INVALID_ARGUMENT, "joint selection matrix is not full rank in JointTask constructor");
		T.dev.m = rows;
		memcpy(T.dev.S, S, sizeof(double) * rows * n);
		bool ident = (rows == n);
		for (int i = 0; i < rows && ident; i++)
			for (int j = 0; j < n; j++)
				if (S[i * n + j] != (i == j ? 1.0 : 0.0)) ident = false;
		T.dev.s_identity = ident;
		T.full_joint = (rows == n);  // JointTask::isFullJointTask(): task dof == robot dof
	}
	for (int i = 0; i < T.dev.m; i++) {  // JointTask.h:32-34
		T.dev.kp[i] = 50.0;
		T.dev.kv[i] = 14.0;
		T.dev.ki[i] = 0.0;
		T.dev.sat[i] = M_PI / 3.0;  // JointTask.h:44
	}
	T.dev.goal_comps = 3 * T.dev.m;
	T.integ_rows = T.dev.m;
	refresh_has_ki(T.dev);
	memset(&T.otg, 0, sizeof(T.otg));
	T.otg.m = T.dev.m;
	T.otg.gs = T.dev.m <= 8 ? 8 : 32;
	for (int i = 0; i < SAIP_MAXN; i++) {
		T.otg_limits[i] = M_PI / 3.0;              // DefaultParameters::otg_max_velocity, JointTask.h:40
		T.otg_limits[SAIP_MAXN + i] = 2.0 * M_PI;  // DefaultParameters::otg_max_acceleration, JointTask.h:41
		T.otg_limits[2 * SAIP_MAXN + i] = 10.0 * M_PI;  // DefaultParameters::otg_max_jerk, JointTask.h:42 (used in jerk-limited mode only)
	}
	b->tasks.push_back(T);
	b->config_dirty = true;
	if (task_id) *task_id = (int)b->tasks.size() - 1;
	return SAIP_OK;
}

template <typename Tp>
static saip_status dev_alloc(saip_batch* b, Tp** p, size_t count) {
	void* v = nullptr;
	HIP_TRY(hipMalloc(&v, count * sizeof(Tp)));
	HIP_TRY(hipMemset(v, 0, count * sizeof(Tp)));
	b->allocs.push_back(v);
	*p = (Tp*)v;
	return SAIP_OK;
}

extern "C" saip_status saip_batch_finalize(saip_batch* b) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "null batch");
	if (b->finalized) return SAIP_OK;
	// RobotController constructor checks, RobotController.cpp:8-66
	if (b->tasks.empty()) return fail(SAIP_ERR_INVALID_ARGUMENT, "RobotController must have at least one task");
	bool closed = false;
	for (size_t i = 0; i < b->tasks.size(); i++) {
		if (b->tasks[i].dev.dt != b->tasks[0].dev.dt) return fail(SAIP_ERR_INVALID_ARGUMENT, "All tasks must have the same loop timestep in RobotController");
		for (size_t j = 0; j < i; j++)
			if (b->tasks[j].name == b->tasks[i].name) return fail(SAIP_ERR_INVALID_ARGUMENT, "Tasks in RobotController must have unique names");
		if (closed)
			return fail(SAIP_ERR_INVALID_ARGUMENT, "task [%s] cannot be added to the controller because it is in the nullspace of a full joint task", b->tasks[i].name.c_str());
		if (b->tasks[i].dev.type == saip::TASK_JOINT && b->tasks[i].full_joint) closed = true;
		// k > n: the reference's thin SVD of the k x n task Jacobian has min(k, n) singular values and SingularityHandler.cpp:78-118
		// reads k of them (undefined behaviour); the per-task interface goes through this batch too, so it is refused with it
		if (b->tasks[i].dev.type == saip::TASK_MOTION_FORCE && b->tasks[i].dev.k > b->model->n)
			return fail(SAIP_ERR_UNSUPPORTED,
						"MotionForceTask [%s] controls %d directions but the robot has only %d dof: the reference's singularity handler is undefined "
						"for a task with more directions than joints; use a partial task (controlled_directions_translation / _rotation) of at most %d directions",
						b->tasks[i].name.c_str(), b->tasks[i].dev.k, b->model->n, b->model->n);
	}
	if (has_device(b)) {
		HIP_TRY(hipSetDevice(b->device));
		HIP_TRY(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
		const size_t n = b->model->n, ld = b->ld;
		saip_status st;
		if ((st = dev_alloc(b, &b->q, n * ld)) || (st = dev_alloc(b, &b->dq, n * ld)) || (st = dev_alloc(b, &b->tau, n * ld)) ||
			(st = dev_alloc(b, &b->status, ld)) || (st = dev_alloc(b, &b->model_dev, 1)) || (st = dev_alloc(b, &b->tasks_dev, b->tasks.size())) ||
			(st = dev_alloc(b, &b->flags.buf, 2 * (ld + 32))))
			return st;
		for (auto& T : b->tasks) {
			if ((st = dev_alloc(b, &T.goal_dev, (size_t)T.dev.goal_comps * ld)) || (st = dev_alloc(b, &T.integ_dev, (size_t)T.integ_rows * ld)) ||
				(st = dev_alloc(b, &T.integ_new_dev, (size_t)T.integ_rows * ld)))
				return st;
			T.dev.goal = T.goal_dev;
			T.dev.integ = T.integ_dev;
			T.dev.integ_new = T.integ_new_dev;
		}
		HIP_TRY(hipMemcpy(b->model_dev, &b->model->dev, sizeof(ModelDev), hipMemcpyHostToDevice));
	}
	b->finalized = true;
	b->config_dirty = true;
	return SAIP_OK;
}

extern "C" int saip_batch_task_count(const saip_batch* b) { return b ? (int)b->tasks.size() : 0; }
extern "C" int saip_batch_task_type(const saip_batch* b, int t) {
	if (!b || t < 0 || t >= (int)b->tasks.size()) return SAIP_TASK_UNDEFINED;
	return b->tasks[t].dev.type;
}
extern "C" const char* saip_batch_task_name(const saip_batch* b, int t) {
	if (!b || t < 0 || t >= (int)b->tasks.size()) return nullptr;
	return b->tasks[t].name.c_str();
}
extern "C" int saip_batch_task_by_name(const saip_batch* b, const char* name) {
	if (!b || !name) return -1;
	for (size_t i = 0; i < b->tasks.size(); i++)
		if (b->tasks[i].name == name) return (int)i;
	return -1;
}
extern "C" int saip_batch_task_dof(const saip_batch* b, int t) {
	if (!b || t < 0 || t >= (int)b->tasks.size()) return 0;
	return b->tasks[t].dev.type == saip::TASK_JOINT ? b->tasks[t].dev.m : b->tasks[t].dev.k;
}
extern "C" int saip_batch_goal_components(const saip_batch* b, int t) {
	if (!b || t < 0 || t >= (int)b->tasks.size()) return 0;
	return b->tasks[t].dev.goal_comps;
}
// projection of a motion-force task (parity tests): P 6x6 row-major, basis 6x6 row-major (first *rank columns valid)
extern "C" saip_status saip_batch_get_task_projection(const saip_batch* b, int t, double* P36, double* basis36, int* rank) {
	saip_status st = check_batch(b, t, "saip_batch_get_task_projection");
	if (st) return st;
	if (t < 0 || b->tasks[t].dev.type != saip::TASK_MOTION_FORCE) return fail(SAIP_ERR_INVALID_ARGUMENT, "task %d is not a MotionForceTask", t);
	if (P36) memcpy(P36, b->tasks[t].P, sizeof(double) * 36);
	if (basis36) memcpy(basis36, b->tasks[t].dev.Bm, sizeof(double) * 36);
	if (rank) *rank = b->tasks[t].dev.k;
	return SAIP_OK;
}

static saip_status set_gain3(double* kp, double* kv, double* ki, const double* p, const double* v, const double* i, int n_gains, const char* who) {
	if (!p || !v || !i) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null gain pointer", who);
	if (n_gains != 1 && n_gains != 3) return fail(SAIP_ERR_INVALID_ARGUMENT, "kp, kv and ki should be of size 1 or 3 in %s", who);
	for (int c = 0; c < n_gains; c++)
		if (p[c] < 0 || v[c] < 0 || i[c] < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "all gains should be positive or zero in %s", who);
	for (int c = 0; c < 3; c++) {
		kp[c] = p[n_gains == 1 ? 0 : c];
		kv[c] = v[n_gains == 1 ? 0 : c];
		ki[c] = i[n_gains == 1 ? 0 : c];
	}
	return SAIP_OK;
}
static void refresh_has_ki(TaskDev& d) {
	// derived fields: pseudo-inverse of the diagonal kv gains (SaiModel::computePseudoInverse), control-law variant
	for (int c = 0; c < 3; c++) {
		d.kvinv_pos[c] = fabs(d.kv_pos[c]) > 1e-6 ? 1.0 / d.kv_pos[c] : 0.0;
		d.kvinv_ori[c] = fabs(d.kv_ori[c]) > 1e-6 ? 1.0 / d.kv_ori[c] : 0.0;
	}
	for (int c = 0; c < d.m; c++) d.kvinv[c] = fabs(d.kv[c]) > 1e-6 ? 1.0 / d.kv[c] : 0.0;
	d.general_law = (d.vel_sat || d.force_dim || d.moment_dim || d.cl_force || d.cl_moment) ? 1 : 0;
	d.has_ki = 0;
	if (d.type == saip::TASK_MOTION_FORCE) {
		for (int c = 0; c < 3; c++)
			if (d.ki_pos[c] != 0 || d.ki_ori[c] != 0) d.has_ki = 1;
	} else {
		for (int c = 0; c < d.m; c++)
			if (d.ki[c] != 0) d.has_ki = 1;
	}
}
static saip_status need_type(saip_batch* b, int t, int type, const char* fn) {
	saip_status st = check_batch(b, t, fn);
	if (st) return st;
	if (t < 0 || b->tasks[t].dev.type != type) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task %d has the wrong type", fn, t);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_pos_control_gains(saip_batch* b, int t, const double* kp, const double* kv, const double* ki, int ng) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, "saip_batch_set_pos_control_gains");
	if (st) return st;
	TaskDev& d = b->tasks[t].dev;
	st = set_gain3(d.kp_pos, d.kv_pos, d.ki_pos, kp, kv, ki, ng, "MotionForceTask::setPosControlGains");
	refresh_has_ki(d);
	b->config_dirty = true;
	return st;
}
extern "C" saip_status saip_batch_set_ori_control_gains(saip_batch* b, int t, const double* kp, const double* kv, const double* ki, int ng) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, "saip_batch_set_ori_control_gains");
	if (st) return st;
	TaskDev& d = b->tasks[t].dev;
	st = set_gain3(d.kp_ori, d.kv_ori, d.ki_ori, kp, kv, ki, ng, "MotionForceTask::setOriControlGains");
	refresh_has_ki(d);
	b->config_dirty = true;
	return st;
}
extern "C" saip_status saip_batch_set_joint_gains(saip_batch* b, int t, const double* kp, const double* kv, const double* ki, int ng) {
	saip_status st = need_type(b, t, saip::TASK_JOINT, "saip_batch_set_joint_gains");
	if (st) return st;
	TaskDev& d = b->tasks[t].dev;
	if (!kp || !kv || !ki) return fail(SAIP_ERR_INVALID_ARGUMENT, "JointTask::setGains: null gain pointer");
	if (ng != 1 && ng != d.m) return fail(SAIP_ERR_INVALID_ARGUMENT, "size of gain vectors inconsistent with number of task dofs in JointTask::setGains");
	for (int c = 0; c < ng; c++)
		if (kp[c] < 0 || kv[c] < 0 || ki[c] < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "gains must be positive or zero in JointTask::setGains");
	for (int c = 0; c < d.m; c++) {
		d.kp[c] = kp[ng == 1 ? 0 : c];
		d.kv[c] = kv[ng == 1 ? 0 : c];
		d.ki[c] = ki[ng == 1 ? 0 : c];
	}
	refresh_has_ki(d);
	b->config_dirty = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_dynamic_decoupling_type(saip_batch* b, int t, int type) {
	saip_status st = check_batch(b, t, "saip_batch_set_dynamic_decoupling_type");
	if (st) return st;
	if (t < 0 || type < 0 || type > 2) return fail(SAIP_ERR_INVALID_ARGUMENT, "Dynamic decoupling type not recognized");
	b->tasks[t].dev.decoupling = type;
	b->config_dirty = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_bie_threshold(saip_batch* b, int t, double thr) {
	saip_status st = check_batch(b, t, "saip_batch_set_bie_threshold");
	if (st) return st;
	if (t < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad task");
	// JointTask clamps negative thresholds to 0 (JointTask.h:372-378); SingularityHandler stores them as-is (SingularityHandler.h:81-86)
	if (thr < 0 && b->tasks[t].dev.type == saip::TASK_JOINT) thr = 0;
	b->tasks[t].dev.bie_threshold = thr;
	b->config_dirty = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_singularity_bounds(saip_batch* b, int t, double s_min, double s_max) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, "saip_batch_set_singularity_bounds");
	if (st) return st;
	if (s_min < 0 || s_max < s_min) return fail(SAIP_ERR_INVALID_ARGUMENT, "singularity bounds must satisfy 0 <= s_min <= s_max");
	b->tasks[t].dev.s_min = s_min;
	b->tasks[t].dev.s_max = s_max;
	b->config_dirty = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_singularity_handling(saip_batch* b, int t, int enabled) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, "saip_batch_set_singularity_handling");
	if (st) return st;
	b->tasks[t].dev.sing_handling = enabled ? 1 : 0;
	b->config_dirty = true;
	return SAIP_OK;
}
// SingularityHandler state of every instance back to "never singular" (SingularityHandler.cpp:55-63); allocates on first use
static saip_status sh_reinit(saip_batch* b, TaskHost& T) {
	if (!T.dev.sh) {
		saip_status st = dev_alloc(b, &T.dev.sh, (size_t)b->ld);
		if (st) return st;
	}
	HIP_TRY(hipMemsetAsync(T.dev.sh, 0, (size_t)b->ld * sizeof(saip::ShState), b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_singularity_strategies(saip_batch* b, int t, int enabled) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, "saip_batch_set_singularity_strategies");
	if (st) return st;
	TaskHost& T = b->tasks[t];
	T.dev.sing_strategies = enabled ? 1 : 0;
	b->config_dirty = true;
	if (enabled && b->finalized && has_device(b)) {
		if ((st = need_ready(b, "saip_batch_set_singularity_strategies"))) return st;
		return sh_reinit(b, T);
	}
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_singularity_gains(saip_batch* b, int t, double kp_type_1, double kv_type_1, double kv_type_2) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, "saip_batch_set_singularity_gains");
	if (st) return st;
	b->tasks[t].dev.sh_kp1 = kp_type_1;
	b->tasks[t].dev.sh_kv1 = kv_type_1;
	b->tasks[t].dev.sh_kv2 = kv_type_2;
	b->config_dirty = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_all_singularities_type1(saip_batch* b, int t, int flag) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, "saip_batch_set_all_singularities_type1");
	if (st) return st;
	b->tasks[t].dev.sh_force_type1 = flag ? 1 : 0;
	b->config_dirty = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_type1_posture(saip_batch* b, int t, const double* q_des, int per_instance) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, "saip_batch_set_type1_posture");
	if (st) return st;
	if (!q_des) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_set_type1_posture: null posture");
	TaskHost& T = b->tasks[t];
	// _q_prior is overwritten with the current posture whenever an instance enters a singular region (SingularityHandler.cpp:232-235):
	// the call only matters for instances that are inside one, which needs the device state
	if (!T.dev.sing_strategies || !T.dev.sh || !b->finalized || !has_device(b)) return SAIP_OK;
	if ((st = need_ready(b, "saip_batch_set_type1_posture"))) return st;
	const int n = b->model->n;
	std::vector<double> host((size_t)b->B * n);
	for (int i = 0; i < b->B; i++)
		for (int j = 0; j < n; j++) host[(size_t)i * n + j] = per_instance ? q_des[(size_t)i * n + j] : q_des[j];
	HIP_TRY(hipMemcpy2DAsync(T.dev.sh, sizeof(saip::ShState), host.data(), (size_t)n * sizeof(double), (size_t)n * sizeof(double), (size_t)b->B,
							 hipMemcpyHostToDevice, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_internal_otg(saip_batch* b, int t, int enabled) {
	saip_status st = check_batch(b, t, "saip_batch_set_internal_otg");
	if (st) return st;
	if (t < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad task");
	TaskHost& T = b->tasks[t];
	if (enabled && !T.otg_enabled) T.otg_inited = false;  // enableInternalOtg* re-initialises a disabled OTG (JointTask.cpp:374-376)
	T.otg_enabled = enabled != 0;
	b->config_dirty = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_otg_acceleration_limited(saip_batch* b, int t, const double* max_velocity, const double* max_acceleration, int count) {
	saip_status st = check_batch(b, t, "saip_batch_set_otg_acceleration_limited");
	if (st) return st;
	if (t < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad task");
	TaskHost& T = b->tasks[t];
	if (T.dev.type == saip::TASK_MOTION_FORCE) {
		// MotionForceTask::enableInternalOtgAccelerationLimited(max_lin_vel, max_lin_acc, max_ang_vel, max_ang_acc), MotionForceTask.cpp:510-523
		if (!max_velocity || !max_acceleration || count != 2)
			return fail(SAIP_ERR_INVALID_ARGUMENT, "motion-force task: pass {linear, angular} max velocities and max accelerations (count = 2)");
		for (int i = 0; i < 2; i++) {
			if (!(max_velocity[i] > 0)) return fail(SAIP_ERR_INVALID_ARGUMENT, "max velocity set to 0 or negative value in some directions in OTG_6dof_cartesian::setMax%sVelocity", i ? "Angular" : "Linear");
			if (!(max_acceleration[i] > 0)) return fail(SAIP_ERR_INVALID_ARGUMENT, "max acceleration set to 0 or negative value in some directions in OTG_6dof_cartesian::setMax%sAcceleration", i ? "Angular" : "Linear");
		}
		for (int i = 0; i < 6; i++) {
			T.otg_limits[i] = max_velocity[i / 3];
			T.otg_limits[SAIP_MAXN + i] = max_acceleration[i / 3];
		}
		T.otg_limits_dirty = true;
		T.otg.epoch++;
		if (!T.otg_enabled || T.otg.jerk) T.otg_inited = false;  // MotionForceTask.cpp:513-515: re-initialised when the OTG was off or jerk-limited
		T.otg.jerk = 0;
		T.otg_enabled = true;
		b->config_dirty = true;
		return SAIP_OK;
	}
	const int m = T.dev.m;
	if (!max_velocity || !max_acceleration || (count != 1 && count != m))
		return fail(SAIP_ERR_INVALID_ARGUMENT, "max velocity or max acceleration vector size not consistent with task dof in JointTask::enableInternalOtgAccelerationLimited");
	for (int i = 0; i < count; i++) {
		if (!(max_velocity[i] > 0)) return fail(SAIP_ERR_INVALID_ARGUMENT, "max velocity cannot be 0 or negative in any directions in OTG_joints::setMaxVelocity");
		if (!(max_acceleration[i] > 0)) return fail(SAIP_ERR_INVALID_ARGUMENT, "max acceleration cannot be 0 or negative in any directions in OTG_joints::setMaxAcceleration");
	}
	for (int i = 0; i < m; i++) {
		T.otg_limits[i] = max_velocity[count == 1 ? 0 : i];
		T.otg_limits[SAIP_MAXN + i] = max_acceleration[count == 1 ? 0 : i];
	}
	T.otg_limits_dirty = true;
	T.otg.epoch++;
	if (!T.otg_enabled || T.otg.jerk) T.otg_inited = false;  // JointTask.cpp:374-376
	T.otg.jerk = 0;
	T.otg_enabled = true;
	b->config_dirty = true;
	return SAIP_OK;
}
// JointTask::enableInternalOtgJerkLimited (JointTask.cpp:383-410; OTG_joints::setMaxVelocity / setMaxAcceleration / setMaxJerk, OTG_joints.cpp:44-86) and
// MotionForceTask::enableInternalOtgJerkLimited (MotionForceTask.cpp:525-545; OTG_6dof_cartesian::setMaxJerk, OTG_6dof_cartesian.cpp:126-136):
// third-order Ruckig profiles on the device (csrc/saip_otg3.h).  The OTG is re-initialised at the current task position when it was off or
// acceleration-limited (:400-402 / :530-532).
extern "C" saip_status saip_batch_set_otg_jerk_limited(saip_batch* b, int t, const double* max_velocity, const double* max_acceleration, const double* max_jerk, int count) {
	saip_status st = check_batch(b, t, "saip_batch_set_otg_jerk_limited");
	if (st) return st;
	if (t < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad task");
	TaskHost& T = b->tasks[t];
	if (T.dev.type == saip::TASK_MOTION_FORCE) {
		if (!max_velocity || !max_acceleration || !max_jerk || count != 2)
			return fail(SAIP_ERR_INVALID_ARGUMENT, "motion-force task: pass {linear, angular} max velocities, max accelerations and max jerks (count = 2)");
		for (int i = 0; i < 2; i++) {
			if (!(max_velocity[i] > 0)) return fail(SAIP_ERR_INVALID_ARGUMENT, "max velocity set to 0 or negative value in some directions in OTG_6dof_cartesian::setMax%sVelocity", i ? "Angular" : "Linear");
			if (!(max_acceleration[i] > 0)) return fail(SAIP_ERR_INVALID_ARGUMENT, "max acceleration set to 0 or negative value in some directions in OTG_6dof_cartesian::setMax%sAcceleration", i ? "Angular" : "Linear");
			if (!(max_jerk[i] > 0)) return fail(SAIP_ERR_INVALID_ARGUMENT, "max jerk set to 0 or negative value in some directions in OTG_6dof_cartesian::setMaxJerk");
		}
		for (int i = 0; i < 6; i++) {
			T.otg_limits[i] = max_velocity[i / 3];
			T.otg_limits[SAIP_MAXN + i] = max_acceleration[i / 3];
			T.otg_limits[2 * SAIP_MAXN + i] = max_jerk[i / 3];
		}
	} else {
		const int m = T.dev.m;
		if (!max_velocity || !max_acceleration || !max_jerk || (count != 1 && count != m))
			return fail(SAIP_ERR_INVALID_ARGUMENT, "max velocity, max acceleration or max jerk vector size not consistent with task dof in JointTask::enableInternalOtgJerkLimited");
		for (int i = 0; i < count; i++) {
			if (!(max_velocity[i] > 0)) return fail(SAIP_ERR_INVALID_ARGUMENT, "max velocity cannot be 0 or negative in any directions in OTG_joints::setMaxVelocity");
			if (!(max_acceleration[i] > 0)) return fail(SAIP_ERR_INVALID_ARGUMENT, "max acceleration cannot be 0 or negative in any directions in OTG_joints::setMaxAcceleration");
			if (!(max_jerk[i] > 0)) return fail(SAIP_ERR_INVALID_ARGUMENT, "max jerk cannot be 0 or negative in any directions in OTG_joints::setMaxJerk");
		}
		for (int i = 0; i < m; i++) {
			T.otg_limits[i] = max_velocity[count == 1 ? 0 : i];
			T.otg_limits[SAIP_MAXN + i] = max_acceleration[count == 1 ? 0 : i];
			T.otg_limits[2 * SAIP_MAXN + i] = max_jerk[count == 1 ? 0 : i];
		}
	}
	T.otg_limits_dirty = true;
	T.otg.epoch++;
	if (!T.otg_enabled || !T.otg.jerk) T.otg_inited = false;
	T.otg.jerk = 1;
	T.otg_enabled = true;
	b->config_dirty = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_velocity_saturation(saip_batch* b, int t, int enabled) {
	saip_status st = check_batch(b, t, "saip_batch_set_velocity_saturation");
	if (st) return st;
	if (t < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad task");
	b->tasks[t].dev.vel_sat = enabled ? 1 : 0;
	refresh_has_ki(b->tasks[t].dev);
	b->config_dirty = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_saturation_velocities(saip_batch* b, int t, const double* v, int nv) {
	saip_status st = check_batch(b, t, "saip_batch_set_saturation_velocities");
	if (st) return st;
	if (t < 0 || (nv > 0 && !v)) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad task or null values");
	TaskDev& d = b->tasks[t].dev;
	if (d.type == saip::TASK_MOTION_FORCE) {
		if (nv != 2) return fail(SAIP_ERR_INVALID_ARGUMENT, "MotionForceTask::enableVelocitySaturation takes a linear and an angular saturation velocity");
		if (v[0] <= 0 || v[1] <= 0)  // MotionForceTask.cpp:773-777
			return fail(SAIP_ERR_INVALID_ARGUMENT, "Velocity saturation values should be strictly positive or zero in MotionForceTask::enableVelocitySaturation");
		d.lin_sat = v[0];
		d.ang_sat = v[1];
	} else {
		if (nv != 1 && nv != d.m)  // JointTask.cpp:423-427
			return fail(SAIP_ERR_INVALID_ARGUMENT, "saturation velocity vector size not consistent with task dof in JointTask::enableVelocitySaturation");
		for (int i = 0; i < nv; i++)
			if (v[i] <= 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "saturation velocity must be positive in JointTask::enableVelocitySaturation");
		for (int i = 0; i < d.m; i++) d.sat[i] = v[nv == 1 ? 0 : i];
	}
	b->config_dirty = true;
	return SAIP_OK;
}
static saip_status launch_reinit_masked(saip_batch* b, int task, int mask);
static saip_status parametrize_space(saip_batch* b, int t, int dim, const double* axis, int* changed, bool moment, const char* who) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, who);
	if (st) return st;
	if (dim < 0 || dim > 3)  // MotionForceTask.cpp:831-835, 864-868
		return fail(SAIP_ERR_INVALID_ARGUMENT, "%s space dimension should be between 0 and 3 in %s", moment ? "Moment" : "Force", who);
	TaskDev& d = b->tasks[t].dev;
	int& cur_dim = moment ? d.moment_dim : d.force_dim;
	double* cur_axis = moment ? d.moment_axis : d.force_axis;
	bool reset = dim != cur_dim;
	if (dim == 1 || dim == 2) {
		if (!axis) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null axis", who);
		double nrm = sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
		if (nrm < 1e-2)  // :838-842, 871-875
			return fail(SAIP_ERR_INVALID_ARGUMENT, "%s axis should be a non singular vector in %s", moment ? "Moment or rot motion" : "Force or motion", who);
		double a[3] = {axis[0] / nrm, axis[1] / nrm, axis[2] / nrm};
		double diff = fabs(a[0] - cur_axis[0]) + fabs(a[1] - cur_axis[1]) + fabs(a[2] - cur_axis[2]);
		reset = reset || diff > 1e-12;
		memcpy(cur_axis, a, sizeof(a));
	}
	cur_dim = dim;
	refresh_has_ki(d);
	b->config_dirty = true;
	if (changed) *changed = reset ? 1 : 0;
	if (reset && b->finalized && b->device >= 0 && b->state_pushed)  // goal := current, integrators := 0 (:846-852, 880-886)
		return launch_reinit_masked(b, t, moment ? 2 : 1);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_parametrize_force_motion_spaces(saip_batch* b, int t, int dim, const double* axis, int* changed) {
	return parametrize_space(b, t, dim, axis, changed, false, "MotionForceTask::parametrizeForceMotionSpaces");
}
extern "C" saip_status saip_batch_parametrize_moment_rot_motion_spaces(saip_batch* b, int t, int dim, const double* axis, int* changed) {
	return parametrize_space(b, t, dim, axis, changed, true, "MotionForceTask::parametrizeMomentRotMotionSpaces");
}
extern "C" saip_status saip_batch_set_parametrization_in_compliant_frame(saip_batch* b, int t, int enabled) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, "saip_batch_set_parametrization_in_compliant_frame");
	if (st) return st;
	b->tasks[t].dev.param_in_compliant_frame = enabled ? 1 : 0;
	b->config_dirty = true;
	return SAIP_OK;
}
static saip_status set_fm_gains(saip_batch* b, int t, double kp, double kv, double ki, bool moment, const char* who) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, who);
	if (st) return st;
	if (kp < 0 || kv < 0 || ki < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "all gains should be positive or zero in %s", who);
	TaskDev& d = b->tasks[t].dev;
	(moment ? d.kv_moment : d.kv_force) = kv;
	(moment ? d.kp_moment : d.kp_force) = kp;  // kp, ki only act in closed-loop control
	(moment ? d.ki_moment : d.ki_force) = ki;
	b->config_dirty = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_force_control_gains(saip_batch* b, int t, double kp, double kv, double ki) {
	return set_fm_gains(b, t, kp, kv, ki, false, "MotionForceTask::setForceControlGains");
}
extern "C" saip_status saip_batch_set_moment_control_gains(saip_batch* b, int t, double kp, double kv, double ki) {
	return set_fm_gains(b, t, kp, kv, ki, true, "MotionForceTask::setMomentControlGains");
}
// setClosedLoopForceControl / setClosedLoopMomentControl (MotionForceTask.cpp:973-986): a change resets the linear / angular integrators
static saip_status set_closed_loop(saip_batch* b, int t, int enabled, bool moment, const char* who) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, who);
	if (st) return st;
	TaskDev& d = b->tasks[t].dev;
	int& flag = moment ? d.cl_moment : d.cl_force;
	const bool changed = (flag != 0) != (enabled != 0);
	flag = enabled ? 1 : 0;
	refresh_has_ki(d);
	b->config_dirty = true;
	if (changed && b->finalized && has_device(b)) {
		// resetIntegratorsLinear / Angular: position + force (orientation + moment) integrators := 0
		const int rows[2] = {moment ? 3 : 0, moment ? 9 : 6};
		for (int r : rows) HIP_TRY(hipMemsetAsync(b->tasks[t].integ_dev + (size_t)r * b->ld, 0, (size_t)3 * b->ld * sizeof(double), b->stream));
		HIP_TRY(hipStreamSynchronize(b->stream));
	}
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_closed_loop_force_control(saip_batch* b, int t, int enabled) {
	return set_closed_loop(b, t, enabled, false, "saip_batch_set_closed_loop_force_control");
}
extern "C" saip_status saip_batch_set_closed_loop_moment_control(saip_batch* b, int t, int enabled) {
	return set_closed_loop(b, t, enabled, true, "saip_batch_set_closed_loop_moment_control");
}
// POPCExplicitForceControl::reInitialize (POPCExplicitForceControl.cpp:10-22) for every instance; allocates the state on first use
static saip_status popc_reinit(saip_batch* b, TaskHost& T) {
	const int cap = T.dev.popc_cap;
	const size_t rows = 7 + (size_t)cap, ld = b->ld;
	if (!T.dev.popc) {
		saip_status st = dev_alloc(b, &T.dev.popc, rows * ld);
		if (st) return st;
	}
	HIP_TRY(hipMemsetAsync(T.dev.popc, 0, rows * ld * sizeof(double), b->stream));
	std::vector<double> one(ld, 1.0), fifty(ld, 50.0);  // _Rc = 1, _PO_counter = _PO_max_counter
	HIP_TRY(hipMemcpyAsync(T.dev.popc + 2 * ld, one.data(), ld * sizeof(double), hipMemcpyHostToDevice, b->stream));
	HIP_TRY(hipMemcpyAsync(T.dev.popc + 4 * ld, fifty.data(), ld * sizeof(double), hipMemcpyHostToDevice, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));
	return SAIP_OK;
}
// enablePassivity / disablePassivity (MotionForceTask.h:630-631 -> POPCExplicitForceControl::enable / disable, .cpp:24-29)
extern "C" saip_status saip_batch_set_passivity(saip_batch* b, int t, int enabled) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, "saip_batch_set_passivity");
	if (st) return st;
	TaskHost& T = b->tasks[t];
	T.dev.popc_enabled = enabled ? 1 : 0;
	if (T.dev.popc_cap == 0) T.dev.popc_cap = 1024;
	b->config_dirty = true;
	if (b->finalized && has_device(b)) {
		if ((st = need_ready(b, "saip_batch_set_passivity"))) return st;
		if (!enabled || !T.dev.popc) return popc_reinit(b, T);  // disable() re-initialises; the first enable() creates the state
	}
	return SAIP_OK;
}
// setFeedforwardForceGain / MomentGain, setMaxForceControlFeedbackOutput / Moment (MotionForceTask.h:330-355)
extern "C" saip_status saip_batch_set_force_control_parameters(saip_batch* b, int t, double kff_force, double kff_moment, double max_force_feedback, double max_moment_feedback) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, "saip_batch_set_force_control_parameters");
	if (st) return st;
	TaskDev& d = b->tasks[t].dev;
	d.kff_force = kff_force;
	d.kff_moment = kff_moment;
	d.max_force_fb = max_force_feedback;
	d.max_moment_fb = max_moment_feedback;
	b->config_dirty = true;
	return SAIP_OK;
}
// setForceSensorFrame (MotionForceTask.cpp:794-803), given directly as _T_control_to_sensor = compliant_frame^-1 * T_link_sensor
extern "C" saip_status saip_batch_set_control_to_sensor_transform(saip_batch* b, int t, const double* R_row_major, const double* translation) {
	saip_status st = need_type(b, t, saip::TASK_MOTION_FORCE, "saip_batch_set_control_to_sensor_transform");
	if (st) return st;
	if (!R_row_major || !translation) return fail(SAIP_ERR_INVALID_ARGUMENT, "null transform");
	TaskDev& d = b->tasks[t].dev;
	for (int i = 0; i < 9; i++) d.Rcs[i] = R_row_major[i];
	for (int i = 0; i < 3; i++) d.tcs[i] = translation[i];
	b->config_dirty = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_enable_gravity_compensation(saip_batch* b, int e) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "null batch");
	b->gravity_comp = e != 0;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_enable_joint_limit_avoidance(saip_batch* b, int e) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "null batch");
	b->jla = e != 0;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_enable_torque_saturation(saip_batch* b, int e) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "null batch");
	b->torque_sat = e != 0;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_flagged_torque_policy(saip_batch* b, int nan) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "null batch");
	b->flag_nan = nan != 0;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_flagged_recompute(saip_batch* b, int on_list) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "null batch");
	b->flagged_on_list = on_list != 0;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_integrator_tracking(saip_batch* b, int always) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "null batch");
	b->integ_always = always != 0;
	return SAIP_OK;
}

// finalized on a device; model-only batches included (state entries and model queries)
static saip_status need_state(saip_batch* b, const char* fn) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null batch", fn);
	if (!b->finalized) return fail(SAIP_ERR_ORDER, "%s: call saip_batch_finalize first", fn);
	if (!has_device(b)) return fail(SAIP_ERR_NO_DEVICE, "%s: configuration-only batch (no HIP device): the engine has no CPU path", fn);
	if (hipSetDevice(b->device) != hipSuccess) return fail(SAIP_ERR_DEVICE, "hipSetDevice(%d) failed", b->device);
	return SAIP_OK;
}
// ... with a controller: every entry that needs a task
static saip_status need_ready(saip_batch* b, const char* fn) {
	if (b && b->finalized && b->model_only) return fail(SAIP_ERR_ORDER, "%s: the batch was finalized for model queries only (no tasks)", fn);
	return need_state(b, fn);
}
// host [comps][B] <-> device [comps][ld]
static saip_status copy_h2d(saip_batch* b, double* dev, const double* host, int comps) {
	HIP_TRY(hipMemcpy2DAsync(dev, (size_t)b->ld * sizeof(double), host, (size_t)b->B * sizeof(double), (size_t)b->B * sizeof(double), comps,
							 hipMemcpyHostToDevice, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));  // the host buffer may be reused by the caller right away
	return SAIP_OK;
}
static saip_status copy_d2h(saip_batch* b, double* host, const double* dev, int comps) {
	HIP_TRY(hipMemcpy2DAsync(host, (size_t)b->B * sizeof(double), dev, (size_t)b->ld * sizeof(double), (size_t)b->B * sizeof(double), comps,
							 hipMemcpyDeviceToHost, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));
	return SAIP_OK;
}

extern "C" saip_status saip_batch_set_state_host(saip_batch* b, const double* q, const double* dq) {
	saip_status st = need_state(b, "saip_batch_set_state_host");
	if (st) return st;
	if (!q || !dq) return fail(SAIP_ERR_INVALID_ARGUMENT, "null state pointer");
	b->models_valid = false;
	b->state_epoch++;
	if ((st = copy_h2d(b, b->q, q, b->model->n))) return st;
	b->state_pushed = true;
	return copy_h2d(b, b->dq, dq, b->model->n);
}
extern "C" saip_status saip_batch_set_goal_host(saip_batch* b, int t, const double* goal) {
	saip_status st = need_ready(b, "saip_batch_set_goal_host");
	if (st) return st;
	if (t < 0 || t >= (int)b->tasks.size() || !goal) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad task id or null goal");
	return copy_h2d(b, b->tasks[t].goal_dev, goal, b->tasks[t].dev.goal_comps);
}
extern "C" saip_status saip_batch_set_goal_field_host(saip_batch* b, int t, int first, int count, const double* values) {
	saip_status st = need_ready(b, "saip_batch_set_goal_field_host");
	if (st) return st;
	if (t < 0 || t >= (int)b->tasks.size() || !values) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad task id or null values");
	if (first < 0 || count <= 0 || first + count > b->tasks[t].dev.goal_comps)  // e.g. JointTask.cpp:110-114
		return fail(SAIP_ERR_INVALID_ARGUMENT, "goal vector size not consistent with task dof");
	return copy_h2d(b, b->tasks[t].goal_dev + (size_t)first * b->ld, values, count);
}
extern "C" saip_status saip_batch_get_goal_host(saip_batch* b, int t, double* goal) {
	saip_status st = need_ready(b, "saip_batch_get_goal_host");
	if (st) return st;
	if (t < 0 || t >= (int)b->tasks.size() || !goal) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad task id or null goal");
	return copy_d2h(b, goal, b->tasks[t].goal_dev, b->tasks[t].dev.goal_comps);
}

extern "C" double* saip_batch_device_q(saip_batch* b) { return b ? b->q : nullptr; }
extern "C" double* saip_batch_device_dq(saip_batch* b) { return b ? b->dq : nullptr; }
extern "C" double* saip_batch_device_goal(saip_batch* b, int t) { return (b && t >= 0 && t < (int)b->tasks.size()) ? b->tasks[t].goal_dev : nullptr; }
extern "C" double* saip_batch_device_tau(saip_batch* b) { return b ? (b->tau_bound ? b->tau_bound : b->tau) : nullptr; }
extern "C" uint8_t* saip_batch_device_status(saip_batch* b) { return b ? b->status : nullptr; }
extern "C" saip_status saip_batch_bind_tau_device(saip_batch* b, double* tau_dev) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "null batch");
	b->tau_bound = tau_dev;
	return SAIP_OK;
}
extern "C" void* saip_batch_stream(saip_batch* b) { return b ? (void*)b->stream : nullptr; }

// lazily allocate the OTG state of a joint task: [fields][B*gs] lane-major doubles + per-instance scalars
static saip_status ensure_otg(saip_batch* b, TaskHost& T) {
	if (T.otg_alloc) return SAIP_OK;
	saip_status st;
	OtgDev& O = T.otg;
	O.lanes = (long long)b->B * O.gs;
	O.dt = T.dev.dt;
	O.n = b->model->n;
	if ((st = dev_alloc(b, &O.state, (size_t)saip::otg_state_fields() * (size_t)O.lanes)) || (st = dev_alloc(b, &O.time, (size_t)b->ld)) ||
		(st = dev_alloc(b, &O.duration, (size_t)b->ld)) || (st = dev_alloc(b, &O.flags, (size_t)b->ld)) || (st = dev_alloc(b, &O.seen_epoch, (size_t)b->ld)) ||
		(st = dev_alloc(b, &O.result, (size_t)b->ld)) || (st = dev_alloc(b, &T.desired_dev, (size_t)T.dev.goal_comps * b->ld)) ||
		(st = dev_alloc(b, &T.otg_limits_dev, (size_t)3 * SAIP_MAXN)))
		return st;
	if (T.dev.type == saip::TASK_MOTION_FORCE && (st = dev_alloc(b, &O.frame, (size_t)21 * b->ld))) return st;
	O.model = b->model_dev;
	O.goal_comps = T.dev.goal_comps;
	O.limits = T.otg_limits_dev;
	T.otg_limits_dirty = true;
	O.desired = T.desired_dev;
	O.goal = T.goal_dev;
	O.q = b->q;
	T.otg_alloc = true;
	T.otg_inited = false;
	return SAIP_OK;
}
// mode 1: OTG_joints::reInitialize(S q) for every instance; mode 0: one cycle of setGoal + update
static saip_status run_otg(saip_batch* b, int t, int mode, int mask = 3) {
	TaskHost& T = b->tasks[t];
	T.otg.goal_comps = T.dev.goal_comps;
	T.otg.task = b->tasks_dev + t;
	T.otg.dt = T.dev.dt;
	if (T.otg_limits_dirty) {
		HIP_TRY(hipMemcpyAsync(T.otg_limits_dev, T.otg_limits, sizeof(T.otg_limits), hipMemcpyHostToDevice, b->stream));
		HIP_TRY(hipStreamSynchronize(b->stream));  // limits change rarely; keeps the host array free to change again
		T.otg_limits_dirty = false;
	}
	hipError_t e = T.dev.type == saip::TASK_JOINT ? saip::launch_otg_joints(T.otg, b->B, b->ld, mode, b->stream)
												  : saip::launch_otg_cartesian(T.otg, b->B, b->ld, mode | (mask << 4), b->model->dev.is_tree != 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "OTG kernel launch failed: %s", hipGetErrorString(e));
	if (mode == 1 && mask == 3) T.otg_inited = true;
	return SAIP_OK;
}

// a motion-force task that controls all of its space in motion: identity projections and, where the short control law is used, identity
// sigma matrices as well
static bool mf_full_identity(const TaskDev& d, bool with_sigma) {
	return m3_is_eye(d.Ppos) && m3_is_eye(d.Pori) && (!with_sigma || (m3_is_eye(d.sig_p) && m3_is_eye(d.sig_o)));
}

// the lazily allocated state arrays every enabled feature needs: what the first cycle would allocate (state snapshots call it too, so
// that a snapshot created before the first cycle has the layout the cycles will use)
static saip_status ensure_lazy_state(saip_batch* b) {
	for (auto& T : b->tasks) {
		if (T.otg_enabled) {
			saip_status st = ensure_otg(b, T);
			if (st) return st;
		}
		if (T.dev.type == saip::TASK_MOTION_FORCE && T.dev.sing_strategies && !T.dev.sh) {  // enabled before finalize
			saip_status st = sh_reinit(b, T);
			if (st) return st;
			b->config_dirty = true;
		}
		if (T.dev.type == saip::TASK_MOTION_FORCE && T.dev.popc_enabled && !T.dev.popc) {  // enabled before finalize
			saip_status st = popc_reinit(b, T);
			if (st) return st;
			b->config_dirty = true;
		}
	}
	return SAIP_OK;
}
static saip_status make_params(saip_batch* b, CycleParams& P, bool diag) {
	{
		saip_status st = ensure_lazy_state(b);
		if (st) return st;
	}
	if (b->config_dirty || diag) {
		std::vector<TaskDev> tmp;
		for (auto& T : b->tasks) {
			TaskDev d = T.dev;
			d.diag_N = diag ? T.diag_dev : nullptr;
			if (T.otg_enabled) d.goal = T.desired_dev;  // the law tracks the OTG output (JointTask.cpp:317-319, MotionForceTask.cpp:394-406)
			d.law_identity = 0;
			if (d.type == saip::TASK_MOTION_FORCE && d.k == 6 && !d.general_law) {
				bool id = mf_full_identity(d, true);
				for (int i = 0; i < 36 && id; i++) id = d.Bm[i] == ((i % 7 == 0) ? 1.0 : 0.0);
				d.law_identity = id ? 1 : 0;
			}
			tmp.push_back(d);
		}
		HIP_TRY(hipMemcpyAsync(b->tasks_dev, tmp.data(), tmp.size() * sizeof(TaskDev), hipMemcpyHostToDevice, b->stream));
		HIP_TRY(hipStreamSynchronize(b->stream));  // tmp is a stack object
		b->config_dirty = diag;  // a diagnostic upload must be replaced before the next normal launch
	}
	P.B = b->B;
	P.ld = b->ld;
	P.n = b->model->n;
	P.nt = (int)b->tasks.size();
	P.sim_substeps = 0;
	P.sim_dt = P.sim_damping = 0.0;
	P.sim_gravity[0] = P.sim_gravity[1] = P.sim_gravity[2] = 0.0;
	P.gravity_comp = b->gravity_comp;
	P.torque_sat = b->torque_sat;
	P.integ_always = b->integ_always;
	P.jla = b->jla;
	P.only_flagged = 0;
	P.diag = diag;
	P.q = b->q;
	P.dq = b->dq;
	P.tau = b->tau_bound ? b->tau_bound : b->tau;
	P.status = b->status;
	if (diag) {
		// a diagnostic launch re-evaluates the task models only (phase 1: no control law, no integrator / OTG / handler / passivity state
		// is advanced) and writes its torques and status to scratch: the results of the last cycle stay what integrate() / getTorques() see
		saip_status st;
		if (!b->diag_tau && ((st = dev_alloc(b, &b->diag_tau, (size_t)b->model->n * b->ld)) || (st = dev_alloc(b, &b->diag_status, (size_t)b->ld)))) return st;
		P.tau = b->diag_tau;
		P.status = b->diag_status;
	}
	P.model = b->model_dev;
	P.tasks = b->tasks_dev;
	for (int t = 0; t < 2; t++) {
		P.goal2[t] = t < (int)b->tasks.size() ? (b->tasks[t].otg_enabled ? b->tasks[t].desired_dev : b->tasks[t].dev.goal) : nullptr;  // (as in the task block uploaded above)
		P.integ2[t] = t < (int)b->tasks.size() ? b->tasks[t].dev.integ : nullptr;
	}
	// lane kernel: motion-force task slots, batch-uniform rank bounds, the shared BIE threshold
	P.mf_task[0] = P.mf_task[1] = -1;
	P.any_bie = 0;
	P.bie_thr = 0.0;
	int nmf = 0, used = 0;
	for (int t = 0; t < SAIP_MAXT; t++) P.rank_bound[t] = P.lane_task_is_joint[t] = 0;
	for (size_t t = 0; t < b->tasks.size(); t++) {
		const TaskDev& d = b->tasks[t].dev;
		int own = d.type == saip::TASK_MOTION_FORCE ? d.k : d.m;
		int bound = own < P.n - used ? own : P.n - used;  // rank(J N_prec) <= n - sum of the ranks certified above
		P.rank_bound[t] = bound < 0 ? 0 : bound;
		P.lane_task_is_joint[t] = d.type == saip::TASK_JOINT;
		if (d.type == saip::TASK_MOTION_FORCE) {
			if (nmf < 2) P.mf_task[nmf] = (int)t;
			nmf++;
			used += d.k;  // exact whenever the instance stays in the non-singular branch (otherwise it is flagged anyway)
		}
		if (d.decoupling == SAIP_BOUNDED_INERTIA_ESTIMATES) {
			P.any_bie = 1;
			P.bie_thr = d.bie_threshold;
		}
	}
	P.reinit_task = -1;
	P.reinit_mask = 7;
	P.single_task = -1;
	P.phase = diag ? 1 : 0;
	P.ext_nprec = nullptr;
	P.ext_tau_prec = nullptr;
	P.out_N = nullptr;
	P.out_Ntot = nullptr;
	for (int t = 0; t < SAIP_MAXT; t++) P.task_cycle[t] = t < (int)b->tasks.size() ? b->tasks[t].sh_cycle : 0;
	P.flag_nan = b->flag_nan ? 1 : 0;
	// neutral: no work list, no slow tail, the lean eight-lane instantiation.  launch_cycle alone overwrites these, from its CyclePlan
	P.flag_count = P.flag_count_next = P.flag_list = nullptr;
	P.slow_tail = P.oct_general_joint = P.oct_partial_mf = P.oct_truncate = 0;
	P.lane_general = 0;
	for (auto& T : b->tasks)
		if (T.dev.general_law) P.lane_general = 1;
	P.wave_general_joint = 0;
	for (size_t t = 0; t < b->tasks.size(); t++) {
		const TaskDev& T = b->tasks[t].dev;
		if (T.type == saip::TASK_JOINT && !(T.s_identity && T.m == P.n && t + 1 == b->tasks.size())) P.wave_general_joint = 1;
	}
	P.lane_prefetch_ok = (b->tasks.size() == 2 && b->tasks[0].dev.type == saip::TASK_MOTION_FORCE && b->tasks[1].dev.type == saip::TASK_JOINT &&
						  b->tasks[1].dev.m == P.n && !b->tasks[0].dev.general_law) ? 1 : 0;
	return SAIP_OK;
}
// the lane-per-instance register kernel covers 6..8 dof, at most two motion-force tasks and one shared BIE threshold
static bool lane_eligible(const saip_batch* b) {
	const int n = b->model->n;
	if (n < 6 || n > 8 || b->model->dev.is_tree) return false;  // (chains only: the fast kernels scan along the chain)
	int nmf = 0;
	double thr = -1.0;
	for (auto& T : b->tasks) {
		if (T.dev.type == saip::TASK_MOTION_FORCE) nmf++;
		// closed-loop force / moment control runs in the lane kernel's general-law instantiations; with the passivity controller around
		// the force loop (per-instance energy window in HBM) the stack stays with the general kernel
		if (T.dev.type == saip::TASK_MOTION_FORCE && (T.dev.cl_force || T.dev.cl_moment) && T.dev.popc_enabled) return false;
		if (T.dev.decoupling == SAIP_BOUNDED_INERTIA_ESTIMATES) {
			if (thr >= 0.0 && thr != T.dev.bie_threshold) return false;
			thr = T.dev.bie_threshold;
		}
	}
	return nmf <= 2;
}
// wavefront-per-instance kernel (saip_kernel_wave.hip): chains of 9..32 dof, any stack of motion-force tasks (rank >= 2) and joint tasks.
// A passivity controller around a force loop keeps its stack on the general kernel: its observer state in HBM is advanced by the control
// law itself, so an instance this kernel flags late in the hierarchy would advance it twice when the general kernel recomputes it.
static bool wave_eligible(const saip_batch* b) {
	const int n = b->model->n;
	if (n <= 8 || n > 32 || b->model->dev.is_tree) return false;
	for (auto& T : b->tasks) {
		if (T.dev.type == saip::TASK_MOTION_FORCE && (T.dev.cl_force || T.dev.cl_moment) && T.dev.popc_enabled) return false;
		if (T.dev.type == saip::TASK_MOTION_FORCE && (T.dev.k < 2 || T.dev.k > 6)) return false;
	}
	return true;
}
// eight-lanes-per-instance kernel (saip_kernel_oct.hip): 7-dof chain, { MotionForceTask, JointTask }.  Either the headline stack
// (full 6-dof motion-force task + full joint task: the joint task has rank <= 1) or any motion-force task of rank >= 2 with a joint
// task of at most four rows (general range basis); default or general control laws, no closed-loop force control.
static OctFit oct_eligible(const saip_batch* b) {  // (on top of lane_eligible)
	OctFit fit;
	const int n = b->model->n;
	if (n < 6 || n > 8 || b->tasks.size() != 2 || b->model->dev.is_tree) return fit;
	const TaskDev& mf = b->tasks[0].dev;
	const TaskDev& jt = b->tasks[1].dev;
	if (mf.type != saip::TASK_MOTION_FORCE || jt.type != saip::TASK_JOINT) return fit;
	if (mf.cl_force || mf.cl_moment || mf.k < 2) return fit;
	const bool full_mf = mf.k == 6 && mf.bm_identity;
	const bool full_jt = jt.m == n && jt.s_identity;
	if (!full_mf && mf.general_law) return fit;  // the general laws are wired for the full task only
	// full task: the projections are identities; the short control law also relies on identity sigma matrices
	if (full_mf && !mf_full_identity(mf, !mf.general_law)) return fit;
	if (n != 7) {
		// 6- and 8-dof chains: the general instantiation only -- full joint task behind a motion-force task, Jp = N_1 of rank n - k (<= 5) by the
		// multi-pivot Gram-Schmidt path; singularity handling on (a reduced task would need the 7-dof bookkeeping), no joint limit avoidance
		if (!full_jt || n - mf.k > 5 || n - mf.k < 0 || !mf.sing_handling || b->jla) return fit;
		fit.general_joint = 2;
	} else {
		const bool full_behind_partial = full_jt && !full_mf && mf.k <= 5;  // Jp = N_1 has rank 7 - k: multi-pivot Gram-Schmidt path
		if (!(full_mf && full_jt) && !full_behind_partial && jt.m > 4) return fit;
		fit.general_joint = (full_mf && full_jt) ? 0 : (full_behind_partial ? 2 : 1);
		if (full_mf && full_jt && !mf.sing_handling && !mf.general_law) {  // disableSingularityHandling(): reduced tasks need the multi-pivot joint-task path
			fit.general_joint = 2;
			fit.truncate = 1;
		}
	}
	fit.partial_mf = full_mf ? 0 : 1;
	fit.ok = true;
	return fit;
}
// eight-lanes-per-instance kernel for hierarchies that START with a joint task (saip_kernel_octjf.hip): 7- or 8-dof chain,
// { JointTask of <= 4 rows, each selecting one joint; full 6-dof MotionForceTask in its nullspace } -- the stack of examples/06.
// Default or general (open-loop) control laws, any decoupling type, gravity compensation, torque saturation; joint limit avoidance and
// closed-loop force control keep the stack on the lane kernel.
static bool octjf_eligible(const saip_batch* b) {  // (on top of lane_eligible)
	const int n = b->model->n;
	if ((n != 7 && n != 8) || b->tasks.size() != 2 || b->jla || b->model->dev.is_tree) return false;
	const TaskDev& jt = b->tasks[0].dev;
	const TaskDev& mf = b->tasks[1].dev;
	if (jt.type != saip::TASK_JOINT || mf.type != saip::TASK_MOTION_FORCE) return false;
	if (jt.m < 1 || jt.m > 4 || n - jt.m < 6) return false;  // (fewer than six joints left: the 6-dof task behind is always singular)
	unsigned seen = 0;
	for (int a = 0; a < jt.m; a++) {  // rows of S: distinct unit vectors (S then has full row rank: matrixRangeBasis returns the identity)
		int hit = -1;
		for (int l = 0; l < n; l++) {
			const double v = jt.S[a * n + l];
			if (v == 1.0 && hit < 0) hit = l;
			else if (v != 0.0) return false;
		}
		if (hit < 0 || (seen >> hit & 1u)) return false;
		seen |= 1u << hit;
	}
	if (mf.k != 6 || !mf.bm_identity || mf.cl_force || mf.cl_moment) return false;  // (goal rows 30..35, the sensed force and moment, are only read by the closed-loop laws)
	return mf_full_identity(mf, false);
}
// both OTGs of a { MotionForceTask, JointTask } stack on, initialised and with clean limits: their cycle-mode steps share one launch
static bool otg_pair_ready(saip_batch* b) {
	if (!(b->tasks.size() == 2 && b->tasks[0].otg_enabled && b->tasks[1].otg_enabled && b->tasks[0].dev.type == saip::TASK_MOTION_FORCE &&
		  b->tasks[1].dev.type == saip::TASK_JOINT && b->tasks[1].otg.gs == 8 && !b->tasks[0].otg_limits_dirty && !b->tasks[1].otg_limits_dirty &&
		  !b->tasks[0].otg.jerk && !b->tasks[1].otg.jerk))
		return false;
	for (int t = 0; t < 2; t++) {
		TaskHost& T = b->tasks[t];
		if (!T.otg_inited) return false;
		T.otg.goal_comps = T.dev.goal_comps;
		T.otg.task = b->tasks_dev + t;
		T.otg.dt = T.dev.dt;
	}
	return true;
}

// ---- which cycle kernel a launch takes, who recomputes the instances it flags, and whether it integrates the state as well: decided
// here and nowhere else.  A pure function of the batch and the parameter block; launch_cycle carries the plan out.
static CyclePlan plan_cycle(const saip_batch* b, const CycleParams& P, bool diag, bool wants_sim) {
	CyclePlan plan;
	const KernelChoice choice = b->kernel_choice;
	auto refuse = [&plan](const char* why) {
		plan.refused = SAIP_ERR_UNSUPPORTED;
		plan.why = why;
		return plan;
	};
	if (diag || choice == KernelChoice::Wg) return plan;  // diagnostic launches always take the general kernel
	const bool lane = lane_eligible(b);
	if (lane) plan.oct = oct_eligible(b);
	const bool octjf_ok = lane && !plan.oct.ok && octjf_eligible(b);
	if (choice == KernelChoice::Oct && !plan.oct.ok && !octjf_ok) return refuse(kOctRefusal);
	if (lane) {
		// small batches of the headline stack: eight lanes per instance (the lane kernel would leave most of the chip idle)
		// Up to which batch: 1024 wavefronts (8192 instances) are resident at once, larger launches run in rounds.  Measured against the lane
		// kernel (round 3): the lean instantiation (config 2's stack) stays ahead up to 24 576 instances (26.8 against
		// 31.1 us) and is level at 32 768; every other instantiation -- partial tasks, reduced tasks, joint task first, 6 / 8 dof -- is ahead
		// at every size (config 3: 109 against 195 us at 65 536, 384 against 627 at 262 144; config 6: 102 against 190 at 65 536), and
		// stacks whose instances leave the non-singular branch are not a contest (the lane kernel hands those to the general kernel).
		const bool oct_lean = plan.oct.ok && plan.oct.general_joint == 0 && !(P.jla || P.lane_general || plan.oct.partial_mf);
		const bool oct_size = !oct_lean || b->B <= 24576;
		const bool eight = choice == KernelChoice::Oct || (choice == KernelChoice::Auto && oct_size);
		plan.kernel = (eight && plan.oct.ok) ? CycleKernel::Oct : ((eight && octjf_ok) ? CycleKernel::OctJf : CycleKernel::Lane);
		// slow path: instances the lane / eight-lane kernel flags (outside the fully non-singular branch) are recomputed by the general kernel
		// when a task can handle them there (blended strategies -- the reference default -- or singularity handling disabled: the task is
		// reduced to its non-singular subspace).  Flagged instances are appended to a list on the device; the general kernel launched
		// behind strides over it with a small fixed grid, no host round trip, and leaves at once when the list is empty.
		bool handled = false;
		for (auto& T : b->tasks)
			if (T.dev.type == saip::TASK_MOTION_FORCE && (!T.dev.sing_handling || T.dev.sing_strategies)) handled = true;
		const bool headline = plan.kernel == CycleKernel::Oct && plan.oct.general_joint == 0;
		if (!handled) plan.recompute = Recompute::None;
		// the eight-lane kernel runs the blended singularity strategies of the headline stack itself (and passes a fully singular task
		// through): with the handling enforced nothing is left for a slow path, and what it still refuses the general kernel would too
		else if (headline && b->tasks[0].dev.sing_handling) plan.recompute = Recompute::None;
		// every other eight-lane stack: the wavefront that flags an instance recomputes it itself behind its epilogue (the general kernel's body on
		// its own LDS block) -- no list and no second launch behind the kernel (round 4)
		else if (plan.kernel != CycleKernel::Lane && !headline && !b->flagged_on_list) plan.recompute = Recompute::Tail;
		else plan.recompute = Recompute::List;
		plan.fuse_sim = wants_sim && headline && plan.recompute == Recompute::None;  // nothing recomputes torques behind this launch: it can integrate as well
		return plan;
	}
	if (choice == KernelChoice::Lane) return refuse(kLaneRefusal);
	const bool wave = wave_eligible(b);
	if (choice == KernelChoice::Wave && !wave) return refuse(kWaveRefusal);
	if (wave) {  // (the choice is Auto or Wave here)
		// chains of 9..32 dof: one wavefront per instance, matrices in MFMA operand form (saip_kernel_wave.hip).  What it cannot certify
		// (a task outside the non-singular branch, an ambiguous rank gap, ...) it leaves untouched on the device-side work list; the
		// general kernel behind recomputes those instances -- an empty list costs that launch one scalar load per workgroup
		plan.kernel = CycleKernel::Wave;
		plan.recompute = Recompute::List;
	}
	return plan;
}

// sim: the integration a rollout would like this launch to do as well; *integrated tells whether it did
static saip_status launch_cycle(saip_batch* b, bool diag, const SimRequest* sim = nullptr, bool* integrated = nullptr) {
	CycleParams P;
	if (!diag)
		for (auto& T : b->tasks) T.sh_cycle++;  // updateControllerTaskModels: every task's model is updated once per cycle
	saip_status st = make_params(b, P, diag);
	if (st) return st;
	for (size_t t = 0; t < b->tasks.size(); t++) {
		TaskHost& T = b->tasks[t];
		if (T.otg_enabled && !T.otg_inited && (st = run_otg(b, (int)t, 1))) return st;
	}
	// { MotionForceTask, JointTask } with both OTGs on: one launch for the two cycle-mode kernels
	bool paired = false;
	if (!diag && otg_pair_ready(b)) {
		if (b->otg_prelaunched) {  // a rollout ran this step together with the previous period's integration
			b->otg_prelaunched = false;
		} else {
			hipError_t e = saip::launch_otg_pair(b->tasks[0].otg, b->tasks[1].otg, b->B, b->ld, b->stream);
			if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "OTG kernel launch failed: %s", hipGetErrorString(e));
		}
		paired = true;
	}
	for (size_t t = 0; t < b->tasks.size() && !paired; t++) {
		TaskHost& T = b->tasks[t];
		if (!T.otg_enabled) continue;
		if (!diag && (st = run_otg(b, (int)t, 0))) return st;  // a diagnostic re-launch must not advance the trajectory
	}
	const CyclePlan plan = plan_cycle(b, P, diag, sim != nullptr);
	if (plan.refused) return fail(plan.refused, "%s", plan.why);
	P.oct_general_joint = plan.oct.general_joint;
	P.oct_partial_mf = plan.oct.partial_mf;
	P.oct_truncate = plan.oct.truncate;
	P.slow_tail = plan.recompute == Recompute::Tail ? 1 : 0;
	if (plan.fuse_sim) {
		P.sim_substeps = sim->substeps;
		P.sim_dt = sim->dt;
		P.sim_damping = sim->damping;
		for (int i = 0; i < 3; i++) P.sim_gravity[i] = sim->gravity[i];
	}
	bool list = plan.recompute == Recompute::List;
	if (list) {
		b->flags.bind(P, b->ld);
		HIP_TRY(b->flags.zero_current(P, b->stream));
	}
	CycleKernel kernel = plan.kernel;
	hipError_t e;
	bool took = true;
	switch (kernel) {
		case CycleKernel::Oct: e = saip::launch_cycle_oct(P, b->stream); break;
		case CycleKernel::OctJf: e = saip::launch_cycle_octjf(P, b->stream); break;
		case CycleKernel::Lane: e = saip::launch_cycle_lane(P, b->stream, &took); break;
		case CycleKernel::Wave: e = saip::launch_cycle_wave(P, b->stream); break;
		default: e = saip::launch_cycle_wg(P, b->model->dev.is_tree != 0, b->stream);
	}
	if (!took) {  // the lane kernel has no instantiation for this stack (there is none such at 6..8 dof): as if the stack were not eligible
		if (b->kernel_choice == KernelChoice::Lane) return fail(SAIP_ERR_UNSUPPORTED, "%s", kLaneRefusal);
		if (b->kernel_choice == KernelChoice::Wave) return fail(SAIP_ERR_UNSUPPORTED, "%s", kWaveRefusal);
		kernel = CycleKernel::Wg;
		list = false;
		e = saip::launch_cycle_wg(P, b->model->dev.is_tree != 0, b->stream);
	}
	if (e != hipSuccess) {
		const char* what = kernel == CycleKernel::Wg ? "kernel" : (kernel == CycleKernel::Wave ? "wavefront-per-instance kernel" : "lane kernel");
		return fail(SAIP_ERR_DEVICE, "%s launch failed: %s", what, hipGetErrorString(e));
	}
	if (list) b->flags.handed_over();
	switch (kernel) {
		case CycleKernel::Oct: b->kernel_name = "saip_cycle_oct"; break;
		case CycleKernel::OctJf: b->kernel_name = "saip_cycle_octjf"; break;
		case CycleKernel::Lane: b->kernel_name = "saip_cycle_lane"; break;
		case CycleKernel::Wave: b->kernel_name = "saip_cycle_wave"; break;
		default:
			if (b->model->dev.is_tree) b->kernel_name = P.n <= 8 ? "saip_cycle_wg_tree<8,64>" : "saip_cycle_wg_tree<32,512>";
			else b->kernel_name = P.n <= 8 ? "saip_cycle_wg<8,64>" : "saip_cycle_wg<32,512>";
	}
	if (list) {
		hipError_t e2 = saip::launch_cycle_wg_list(P, b->stream);
		if (e2 != hipSuccess) return fail(SAIP_ERR_DEVICE, "slow-path kernel launch failed: %s", hipGetErrorString(e2));
	}
	if (integrated) *integrated = plan.fuse_sim;
	return SAIP_OK;
}

static saip_status launch_reinit_masked(saip_batch* b, int task, int mask) {
	std::vector<bool> otg;
	for (auto& T : b->tasks) otg.push_back(T.otg_enabled), T.otg_enabled = false;  // reinit does not depend on the OTG flag
	CycleParams P;
	saip_status st = make_params(b, P, false);
	bool any_otg = false;
	for (size_t i = 0; i < b->tasks.size(); i++) {
		b->tasks[i].otg_enabled = otg[i];
		any_otg = any_otg || otg[i];
	}
	if (any_otg) b->config_dirty = true;  // the upload above pointed the tasks at the raw goal rows: the next cycle must re-point them at the OTG output
	if (st) return st;
	P.reinit_task = task;
	P.reinit_mask = mask;
	hipError_t e = saip::launch_reinit(P, b->model->dev.is_tree != 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "reinit launch failed: %s", hipGetErrorString(e));
	for (size_t t = 0; t < b->tasks.size(); t++) {  // JointTask::reInitializeTask -> _otg->reInitialize (JointTask.cpp:106)
		TaskHost& T = b->tasks[t];
		if ((task >= 0 && (int)t != task) || !T.otg_enabled) continue;
		const int m3 = T.dev.type == saip::TASK_JOINT ? ((mask & 1) ? 3 : 0) : (mask & 3);  // linear / angular parts (reInitializeLinear / Angular)
		if (m3 == 0) continue;
		if ((st = ensure_otg(b, T))) return st;
		if (m3 != 3 && !T.otg_inited && (st = run_otg(b, (int)t, 1, 3))) return st;
		if ((st = run_otg(b, (int)t, 1, m3))) return st;
	}
	HIP_TRY(hipStreamSynchronize(b->stream));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_reinitialize_tasks(saip_batch* b) {
	saip_status st = need_ready(b, "saip_batch_reinitialize_tasks");
	if (st) return st;
	return launch_reinit_masked(b, -1, 7);
}

// MotionForceTask::getCurrentPosition / getCurrentOrientation (MotionForceTask.h:121-138) for the state last pushed: pos [3][B], rot [9][B]
extern "C" saip_status saip_batch_get_current_pose_host(saip_batch* b, int task, double* pos, double* rot) {
	saip_status st = need_type(b, task, saip::TASK_MOTION_FORCE, "saip_batch_get_current_pose_host");
	if (st) return st;
	if ((st = need_ready(b, "saip_batch_get_current_pose_host"))) return st;
	if (!b->pose_dev && (st = dev_alloc(b, &b->pose_dev, (size_t)12 * b->ld))) return st;
	CycleParams P;
	if ((st = make_params(b, P, false))) return st;
	hipError_t e = saip::launch_pose(P, task, b->pose_dev, b->model->dev.is_tree != 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "pose kernel launch failed: %s", hipGetErrorString(e));
	HIP_TRY(hipStreamSynchronize(b->stream));
	if (pos && (st = copy_d2h(b, pos, b->pose_dev, 3))) return st;
	if (rot && (st = copy_d2h(b, rot, b->pose_dev + 3 * (size_t)b->ld, 9))) return st;
	return SAIP_OK;
}
// task diagnostics of one motion-force task (saip_task_diag.hip) for the state last pushed, into out_dev [24][ld] on the batch stream
static saip_status launch_task_diagnostics(saip_batch* b, int task, double* out_dev, const char* fn) {
	saip_status st = need_type(b, task, saip::TASK_MOTION_FORCE, fn);
	if (st) return st;
	if ((st = need_ready(b, fn))) return st;
	if (!out_dev) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null output", fn);
	CycleParams P;
	if ((st = make_params(b, P, false))) return st;
	TaskHost& T = b->tasks[task];
	const bool otg = T.otg_enabled && T.otg_alloc && T.otg_inited;  // as saip_batch_get_desired_host
	hipError_t e = saip::launch_task_diag(P, task, T.goal_dev, otg ? T.desired_dev : T.goal_dev, T.dev.goal_comps, out_dev, b->model->dev.is_tree != 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "task diagnostics kernel launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_get_task_diagnostics_host(saip_batch* b, int task, double* out) {
	const char* fn = "saip_batch_get_task_diagnostics_host";
	saip_status st = need_type(b, task, saip::TASK_MOTION_FORCE, fn);
	if (st) return st;
	if ((st = need_ready(b, fn))) return st;
	if (!out) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null output", fn);
	if (!b->task_diag_dev && (st = dev_alloc(b, &b->task_diag_dev, (size_t)24 * b->ld))) return st;
	if ((st = launch_task_diagnostics(b, task, b->task_diag_dev, fn))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));
	return copy_d2h(b, out, b->task_diag_dev, 24);
}
extern "C" saip_status saip_batch_task_diagnostics_device(saip_batch* b, int task, double* out_dev) {
	return launch_task_diagnostics(b, task, out_dev, "saip_batch_task_diagnostics_device");
}
extern "C" saip_status saip_batch_reinitialize_task(saip_batch* b, int task) {
	saip_status st = need_ready(b, "saip_batch_reinitialize_task");
	if (st) return st;
	if (task < 0 || task >= (int)b->tasks.size()) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_reinitialize_task: bad task");
	return launch_reinit_masked(b, task, 7);
}
// MotionForceTask::resetIntegrators / Linear / Angular (MotionForceTask.cpp:988-1002), JointTask::resetIntegrators: parts bit 0 = linear
// (or the joint task's), bit 1 = angular
extern "C" saip_status saip_batch_reset_integrators(saip_batch* b, int task, int parts) {
	saip_status st = need_ready(b, "saip_batch_reset_integrators");
	if (st) return st;
	if (task < 0 || task >= (int)b->tasks.size()) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_reset_integrators: bad task");
	TaskHost& T = b->tasks[task];
	if (!T.integ_dev) return SAIP_OK;
	const size_t row = (size_t)b->ld * sizeof(double);
	if (T.dev.type == saip::TASK_JOINT) {
		if (parts & 1) HIP_TRY(hipMemsetAsync(T.integ_dev, 0, row * T.dev.m, b->stream));
	} else {
		if (parts & 1) HIP_TRY(hipMemsetAsync(T.integ_dev, 0, row * 3, b->stream));                      // position, then force (rows 6..8)
		if (parts & 1) HIP_TRY(hipMemsetAsync(T.integ_dev + 6 * (size_t)b->ld, 0, row * 3, b->stream));
		if (parts & 2) HIP_TRY(hipMemsetAsync(T.integ_dev + 3 * (size_t)b->ld, 0, row * 3, b->stream));  // orientation, then moment (rows 9..11)
		if (parts & 2) HIP_TRY(hipMemsetAsync(T.integ_dev + 9 * (size_t)b->ld, 0, row * 3, b->stream));
	}
	return SAIP_OK;
}

extern "C" saip_status saip_batch_update_task_models(saip_batch* b) {
	saip_status st = need_ready(b, "saip_batch_update_task_models");
	if (st) return st;
	// The task models are a pure function of the state set by saip_batch_set_state_host; the fused cycle kernel
	// evaluates them together with the control law when computeControlTorques is called (goals may still change).
	b->models_valid = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_step_async(saip_batch* b) {
	saip_status st = need_ready(b, "saip_batch_step_async");
	if (st) return st;
	return launch_cycle(b, false);
}
extern "C" saip_status saip_batch_synchronize(saip_batch* b) {
	saip_status st = need_state(b, "saip_batch_synchronize");
	if (st) return st;
	// A blocking wait.  Polling hipStreamQuery returns ~1 us after the last kernel instead of 4 - 5, but a caller that follows up with ANOTHER
	// runtime wait (hipDeviceSynchronize, torch.cuda.synchronize) then pays for that one's own marker round trip (~19 us instead of ~4 after a
	// blocking wait) -- measured with bench.py at 20 steps: 10.2 us per step polling, 9.7 blocking.
	HIP_TRY(hipStreamSynchronize(b->stream));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_get_torques_host(saip_batch* b, double* tau_host, uint8_t* status_host) {
	saip_status st = need_ready(b, "saip_batch_get_torques_host");
	if (st) return st;
	if (tau_host && (st = copy_d2h(b, tau_host, b->tau_bound ? b->tau_bound : b->tau, b->model->n))) return st;
	if (status_host) {
		HIP_TRY(hipMemcpyAsync(status_host, b->status, b->B, hipMemcpyDeviceToHost, b->stream));
		HIP_TRY(hipStreamSynchronize(b->stream));
	}
	return SAIP_OK;
}
extern "C" saip_status saip_batch_compute_control_torques(saip_batch* b, double* tau_host, uint8_t* status_host) {
	saip_status st = need_ready(b, "saip_batch_compute_control_torques");
	if (st) return st;
	if (!b->models_valid)
		return fail(SAIP_ERR_ORDER, "computeControlTorques: the robot state changed since the last updateControllerTaskModels (stale task models are not supported)");
	if ((st = launch_cycle(b, false))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));
	return saip_batch_get_torques_host(b, tau_host, status_host);
}
extern "C" saip_status saip_batch_get_task_nullspace_host(saip_batch* b, int t, double* N) {
	saip_status st = need_ready(b, "saip_batch_get_task_nullspace_host");
	if (st) return st;
	if (t < 0 || t >= (int)b->tasks.size() || !N) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad task id or null output");
	const int n = b->model->n;
	TaskHost& T = b->tasks[t];
	if (!T.diag_dev && (st = dev_alloc(b, &T.diag_dev, (size_t)n * n * b->ld))) return st;
	// the diagnostic pass re-evaluates the models only (make_params: phase 1, scratch outputs): no state of the batch is advanced
	st = launch_cycle(b, true);
	b->config_dirty = true;
	if (st) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));
	return copy_d2h(b, N, T.diag_dev, n * n);
}
// ------------------------------------------------------------------ per-task entry points, TemplateTask.h:43-60
// The reference's plug-in interface: a caller that builds its own hierarchy drives each task by hand
// (examples/04-task_and_redundancy/04-task_and_redundancy.cpp:141-206): updateTaskModel(N_prec), N_prec = getTaskAndPreviousNullspace(),
// computeTorques() / computeTorques(tau_prec).  One launch of the general kernel per call, restricted to the task.
static saip_status ensure_task_buffers(saip_batch* b, TaskHost& T) {
	if (T.tstatus_dev) return SAIP_OK;
	const size_t n = b->model->n, ld = b->ld;
	saip_status st;
	if ((st = dev_alloc(b, &T.nprec_dev, n * n * ld)) || (st = dev_alloc(b, &T.ntask_dev, n * n * ld)) || (st = dev_alloc(b, &T.ntot_dev, n * n * ld)) ||
		(st = dev_alloc(b, &T.ttau_dev, n * ld)) || (st = dev_alloc(b, &T.tprec_dev, n * ld)) || (st = dev_alloc(b, &T.tstatus_dev, ld)))
		return st;
	return SAIP_OK;
}
static saip_status launch_task(saip_batch* b, int t, int phase, const double* tau_prec_dev, double* tau_out_dev) {
	CycleParams P;
	saip_status st = make_params(b, P, false);
	if (st) return st;
	TaskHost& T = b->tasks[t];
	if (phase == 1) P.task_cycle[t] = ++T.sh_cycle;
	if (phase == 2 && T.otg_enabled) {
		// computeTorques steps the task's internal OTG (JointTask.cpp:313-319, MotionForceTask.cpp:394-406); updateTaskModel does not
		if (!T.otg_inited && (st = run_otg(b, t, 1))) return st;
		if ((st = run_otg(b, t, 0))) return st;
	}
	P.single_task = t;
	P.phase = phase;
	P.rank_bound[t] = T.dev.type == saip::TASK_JOINT ? T.dev.m : T.dev.k;  // N_prec is the caller's: nothing is known about the ranks above
	P.ext_nprec = T.nprec_identity ? nullptr : T.nprec_dev;
	P.ext_tau_prec = phase == 2 ? tau_prec_dev : nullptr;
	P.out_N = phase == 1 ? T.ntask_dev : nullptr;
	P.out_Ntot = phase == 1 ? T.ntot_dev : nullptr;
	P.tau = tau_out_dev ? tau_out_dev : T.ttau_dev;
	P.status = T.tstatus_dev;
	hipError_t e = saip::launch_cycle_wg(P, b->model->dev.is_tree != 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "per-task kernel launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}
static saip_status task_ready(saip_batch* b, int t, const char* fn) {
	saip_status st = need_ready(b, fn);
	if (st) return st;
	if (t < 0 || t >= (int)b->tasks.size()) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, t);
	if (!b->state_pushed) return fail(SAIP_ERR_ORDER, "%s: no robot state has been set (saip_batch_set_state_host)", fn);
	return ensure_task_buffers(b, b->tasks[t]);
}
static saip_status task_update_model(saip_batch* b, int t) {
	saip_status st = launch_task(b, t, 1, nullptr, nullptr);
	if (st) return st;
	b->tasks[t].model_epoch = b->state_epoch;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_task_update_model(saip_batch* b, int t, const double* N_prec_host) {
	saip_status st = task_ready(b, t, "saip_batch_task_update_model");
	if (st) return st;
	TaskHost& T = b->tasks[t];
	T.nprec_identity = N_prec_host == nullptr;
	if (N_prec_host && (st = copy_h2d(b, T.nprec_dev, N_prec_host, b->model->n * b->model->n))) return st;
	return task_update_model(b, t);
}
extern "C" saip_status saip_batch_task_update_model_device(saip_batch* b, int t, const double* N_prec_dev) {
	saip_status st = task_ready(b, t, "saip_batch_task_update_model_device");
	if (st) return st;
	TaskHost& T = b->tasks[t];
	T.nprec_identity = N_prec_dev == nullptr;
	if (N_prec_dev && N_prec_dev != T.nprec_dev)  // the task keeps its own copy like the reference (_N_prec = N_prec)
		HIP_TRY(hipMemcpyAsync(T.nprec_dev, N_prec_dev, (size_t)b->model->n * b->model->n * b->ld * sizeof(double), hipMemcpyDeviceToDevice, b->stream));
	return task_update_model(b, t);
}
static saip_status task_model_fresh(saip_batch* b, int t, const char* fn) {
	if (b->tasks[t].model_epoch != b->state_epoch)
		return fail(SAIP_ERR_ORDER, "%s: task [%s] has no model for the current robot state: call updateTaskModel(N_prec) first (stale task models are not supported)",
					fn, b->tasks[t].name.c_str());
	return SAIP_OK;
}
extern "C" saip_status saip_batch_task_compute_torques_device(saip_batch* b, int t, const double* tau_prec_dev, double* tau_dev) {
	saip_status st = task_ready(b, t, "saip_batch_task_compute_torques_device");
	if (st || (st = task_model_fresh(b, t, "computeTorques"))) return st;
	return launch_task(b, t, 2, tau_prec_dev, tau_dev);
}
extern "C" saip_status saip_batch_task_compute_torques(saip_batch* b, int t, const double* tau_prec_host, double* tau_host, uint8_t* status_host) {
	saip_status st = task_ready(b, t, "saip_batch_task_compute_torques");
	if (st || (st = task_model_fresh(b, t, "computeTorques"))) return st;
	TaskHost& T = b->tasks[t];
	if (tau_prec_host && (st = copy_h2d(b, T.tprec_dev, tau_prec_host, b->model->n))) return st;
	if ((st = launch_task(b, t, 2, tau_prec_host ? T.tprec_dev : nullptr, nullptr))) return st;
	if (tau_host && (st = copy_d2h(b, tau_host, T.ttau_dev, b->model->n))) return st;
	if (status_host) HIP_TRY(hipMemcpyAsync(status_host, T.tstatus_dev, b->B, hipMemcpyDeviceToHost, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));
	return SAIP_OK;
}
extern "C" const double* saip_batch_task_device_nullspace(saip_batch* b, int t, int which) {
	if (!b || t < 0 || t >= (int)b->tasks.size() || b->tasks[t].model_epoch < 0) return nullptr;
	const TaskHost& T = b->tasks[t];
	return which == 0 ? T.ntask_dev : (which == 1 ? (T.nprec_identity ? nullptr : T.nprec_dev) : (which == 2 ? T.ntot_dev : nullptr));
}
extern "C" double* saip_batch_task_device_torques(saip_batch* b, int t) {
	return (b && t >= 0 && t < (int)b->tasks.size()) ? b->tasks[t].ttau_dev : nullptr;
}
extern "C" saip_status saip_batch_task_get_nullspaces_host(saip_batch* b, int t, double* N, double* N_prec, double* N_total) {
	saip_status st = task_ready(b, t, "saip_batch_task_get_nullspaces_host");
	if (st) return st;
	TaskHost& T = b->tasks[t];
	if (T.model_epoch < 0) return fail(SAIP_ERR_ORDER, "task [%s]: updateTaskModel has not been called", T.name.c_str());
	const int n = b->model->n;
	if (N && (st = copy_d2h(b, N, T.ntask_dev, n * n))) return st;
	if (N_total && (st = copy_d2h(b, N_total, T.ntot_dev, n * n))) return st;
	if (N_prec) {
		if (T.nprec_identity) {
			for (int i = 0; i < n; i++)
				for (int j = 0; j < n; j++)
					for (int k = 0; k < b->B; k++) N_prec[((size_t)i * n + j) * b->B + k] = (i == j) ? 1.0 : 0.0;
		} else if ((st = copy_d2h(b, N_prec, T.nprec_dev, n * n))) {
			return st;
		}
	}
	return SAIP_OK;
}
// resident state shared between batches (tasks driven by hand live in batches of their own): device-to-device copy of q, dq [dof][ld]
extern "C" saip_status saip_batch_set_state_device(saip_batch* b, const double* q_dev, const double* dq_dev) {
	saip_status st = need_state(b, "saip_batch_set_state_device");
	if (st) return st;
	if (!q_dev || !dq_dev) return fail(SAIP_ERR_INVALID_ARGUMENT, "null state pointer");
	const size_t bytes = (size_t)b->model->n * b->ld * sizeof(double);
	b->models_valid = false;
	b->state_epoch++;
	if (q_dev != b->q) HIP_TRY(hipMemcpyAsync(b->q, q_dev, bytes, hipMemcpyDeviceToDevice, b->stream));
	if (dq_dev != b->dq) HIP_TRY(hipMemcpyAsync(b->dq, dq_dev, bytes, hipMemcpyDeviceToDevice, b->stream));
	b->state_pushed = true;
	return SAIP_OK;
}
// everything enqueued so far on `producer`'s stream happens before what is enqueued on `waiter`'s stream from now on (device-side
// ordering, no host synchronisation): lets one batch consume device arrays another batch has just written
extern "C" saip_status saip_batch_wait_for(saip_batch* waiter, saip_batch* producer) {
	saip_status st = need_state(waiter, "saip_batch_wait_for");
	if (st || (st = need_state(producer, "saip_batch_wait_for"))) return st;
	if (waiter == producer) return SAIP_OK;
	if (waiter->device != producer->device) return fail(SAIP_ERR_UNSUPPORTED, "saip_batch_wait_for: batches live on different devices");
	if (!producer->sync_event) HIP_TRY(hipEventCreateWithFlags(&producer->sync_event, hipEventDisableTiming));
	HIP_TRY(hipEventRecord(producer->sync_event, producer->stream));
	HIP_TRY(hipStreamWaitEvent(waiter->stream, producer->sync_event, 0));
	return SAIP_OK;
}

extern "C" saip_status saip_batch_set_kernel(saip_batch* b, int which) {
	if (!b || which < 0 || which > 4) return fail(SAIP_ERR_INVALID_ARGUMENT, "kernel selector must be 0, 1, 2, 3 or 4");
	if (which >= 2 && b->model->dev.is_tree)
		return fail(SAIP_ERR_UNSUPPORTED, "saip_batch_set_kernel(%d): this robot is a kinematic tree; only the general kernel (0 or 1) covers trees", which);
	b->kernel_choice = (KernelChoice)which;
	return SAIP_OK;
}
extern "C" const char* saip_batch_kernel_name(saip_batch* b) { return b ? b->kernel_name.c_str() : ""; }

// ---- contact planes and the simulated force sensor (saip_contact.hip): the resident simulator gets something to touch
static saip_status need_controller(const saip_batch* b, const char* fn);
static saip_status need_contact(const saip_batch* b, const char* fn) {
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!b->contact.attached) return fail(SAIP_ERR_ORDER, "%s: no contact planes are attached (saip_batch_contact_attach)", fn);
	return SAIP_OK;
}
static void contact_free(saip_batch* b) {
	auto& C = b->contact;
	for (void* p : {(void*)C.planes, (void*)C.tau_sim, (void*)C.readout, (void*)C.summary})
		if (p) (void)hipFree(p);
	C = saip_batch::Contact();
}
// the plane table as the device keeps it: [P][8] or [P][8][B] with every normal normalised; nullptr: fine, else what is wrong
static const char* contact_check_planes(const double* planes, int P, size_t cols, std::vector<double>& out) {
	out.assign(planes, planes + (size_t)P * saip::CONTACT_PLANE_WORDS * cols);
	for (size_t i = 0; i < out.size(); i++)
		if (!std::isfinite(out[i])) return "a plane value is not finite";
	for (int k = 0; k < P; k++)
		for (size_t i = 0; i < cols; i++) {
			double* w = out.data() + (size_t)k * saip::CONTACT_PLANE_WORDS * cols + i;
			const double nn = std::sqrt(w[0] * w[0] + w[cols] * w[cols] + w[2 * cols] * w[2 * cols]);
			if (!(nn > 0) || !std::isfinite(nn)) return "a plane normal is zero";
			for (int e = 0; e < 3; e++) w[e * cols] /= nn;
			if (!(w[4 * cols] > 0)) return "stiffness k > 0 required";
			if (!(w[5 * cols] >= 0)) return "damping c >= 0 required";
			if (!(w[6 * cols] >= 0)) return "friction mu >= 0 required";
			if (!(w[7 * cols] > 0)) return "slip-regularisation speed v_s > 0 required";
		}
	return nullptr;
}
static saip_status contact_upload_planes(saip_batch* b, double* dev, const std::vector<double>& host, int P, int per_instance, const char* fn) {
	const size_t rows = (size_t)P * saip::CONTACT_PLANE_WORDS;
	hipError_t e;
	if (per_instance)
		e = hipMemcpy2DAsync(dev, (size_t)b->ld * sizeof(double), host.data(), (size_t)b->B * sizeof(double), (size_t)b->B * sizeof(double), rows,
							 hipMemcpyHostToDevice, b->stream);
	else e = hipMemcpyAsync(dev, host.data(), rows * sizeof(double), hipMemcpyHostToDevice, b->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(b->stream);  // `host` goes out of scope with the caller
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "%s: plane upload failed: %s", fn, hipGetErrorString(e));
	return SAIP_OK;
}
static bool contact_rows_overlap(int first, int count) { return first < 36 && first + count > 30; }
// what saip_batch_contact_attach and saip_batch_contact_patch_attach ask of their arguments alike: the carrier ...
static saip_status contact_attach_task(const saip_batch* b, int task, const char* fn) {
	if (task < 0 || task >= (int)b->tasks.size()) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, task);
	if (b->tasks[task].dev.type != saip::TASK_MOTION_FORCE) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task %d is not a motion-force task", fn, task);
	return SAIP_OK;
}
// ... and the planes, the array sizes and the sensor against the task's goal schedule; `host` receives the table as the device keeps it
static saip_status contact_attach_planes(const saip_batch* b, int task, int n_planes, const double* planes, int per_instance, int sensor,
										 std::vector<double>& host, const char* fn) {
	if (n_planes < 1 || n_planes > saip::CONTACT_MAX_PLANES) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: 1..%d planes required (got %d)", fn, saip::CONTACT_MAX_PLANES, n_planes);
	if (!planes) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null planes", fn);
	// [n][ld], [P][8][ld] doubles: the byte counts must fit a size_t
	const size_t widest = (size_t)(b->model->n > 32 ? b->model->n : 32) * sizeof(double);
	if ((size_t)b->ld > SIZE_MAX / widest) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: arrays of leading dimension %d are too large", fn, b->ld);
	if (const char* bad = contact_check_planes(planes, n_planes, per_instance ? (size_t)b->B : 1, host)) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, bad);
	if (sensor && task < (int)b->sched.size() && b->sched[task].attached && contact_rows_overlap(b->sched[task].first, b->sched[task].count))
		return fail(SAIP_ERR_ORDER, "%s: the goal schedule of task %d covers sensed-wrench rows 30..35, which the simulated sensor writes", fn, task);
	return SAIP_OK;
}
// a zeroed device array of `count` doubles; *p stays null when either call fails
static saip_status contact_alloc_zero(saip_batch* b, double** p, size_t count) {
	HIP_TRY(hipMalloc((void**)p, count * sizeof(double)));
	const hipError_t e = hipMemsetAsync(*p, 0, count * sizeof(double), b->stream);
	if (e != hipSuccess) {
		(void)hipFree(*p);
		*p = nullptr;
		return fail(SAIP_ERR_DEVICE, "hipMemsetAsync failed: %s", hipGetErrorString(e));
	}
	return SAIP_OK;
}
extern "C" saip_status saip_batch_contact_attach(saip_batch* b, int task, const double* r_c, int n_planes, const double* planes, int per_instance,
												 int sensor) {
	const char* fn = "saip_batch_contact_attach";
	saip_status st = need_controller(b, fn);
	if (st || (st = contact_attach_task(b, task, fn))) return st;
	if (b->contact.attached) return fail(SAIP_ERR_ORDER, "%s: contact planes are already attached (saip_batch_contact_detach first)", fn);
	if (b->n_patch > 0) return fail(SAIP_ERR_ORDER, "%s: a contact patch is attached (saip_batch_contact_patch_detach first)", fn);
	per_instance = per_instance ? 1 : 0;
	sensor = sensor ? 1 : 0;
	double rc[3] = {0, 0, 0};
	for (int e = 0; e < 3 && r_c; e++) {
		if (!std::isfinite(r_c[e])) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the contact point is not finite", fn);
		rc[e] = r_c[e];
	}
	std::vector<double> host;
	if ((st = contact_attach_planes(b, task, n_planes, planes, per_instance, sensor, host, fn)) || (st = need_ready(b, fn))) return st;
	auto& C = b->contact;
	const size_t ld = b->ld, rows = (size_t)n_planes * saip::CONTACT_PLANE_WORDS;
	if ((st = contact_alloc_zero(b, &C.planes, rows * (per_instance ? ld : 1))) || (st = contact_alloc_zero(b, &C.tau_sim, (size_t)b->model->n * ld)) ||
		(st = contact_alloc_zero(b, &C.readout, (size_t)saip::CONTACT_READOUT_ROWS * ld)) || (st = contact_alloc_zero(b, &C.summary, (size_t)saip::CONTACT_SUMMARY_ROWS * ld)) ||
		(st = contact_upload_planes(b, C.planes, host, n_planes, per_instance, fn))) {
		contact_free(b);
		return st;
	}
	C.attached = true;
	C.task = task;
	C.n_planes = n_planes;
	C.per_instance = per_instance;
	C.sensor = sensor;
	for (int e = 0; e < 3; e++) C.rc[e] = rc[e];
	b->otg_prelaunched = false;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_contact_detach(saip_batch* b) {
	const char* fn = "saip_batch_contact_detach";
	saip_status st = need_contact(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));  // a contact substep may still be in flight
	contact_free(b);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_contact_info(saip_batch* b, int* task, int* n_planes, int* per_instance, int* sensor, double* r_c) {
	saip_status st = need_contact(b, "saip_batch_contact_info");
	if (st) return st;
	const auto& C = b->contact;
	if (task) *task = C.task;
	if (n_planes) *n_planes = C.n_planes;
	if (per_instance) *per_instance = C.per_instance;
	if (sensor) *sensor = C.sensor;
	for (int e = 0; e < 3 && r_c; e++) r_c[e] = C.rc[e];
	return SAIP_OK;
}
extern "C" saip_status saip_batch_contact_set_planes_host(saip_batch* b, const double* planes) {
	const char* fn = "saip_batch_contact_set_planes_host";
	saip_status st = need_contact(b, fn);
	if (st) return st;
	if (!planes) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null planes", fn);
	const auto& C = b->contact;
	std::vector<double> host;
	if (const char* bad = contact_check_planes(planes, C.n_planes, C.per_instance ? (size_t)b->B : 1, host)) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, bad);
	if ((st = need_ready(b, fn))) return st;
	return contact_upload_planes(b, C.planes, host, C.n_planes, C.per_instance, fn);
}
extern "C" double* saip_batch_contact_planes_device(saip_batch* b) { return b ? b->contact.planes : nullptr; }
extern "C" double* saip_batch_contact_torques_device(saip_batch* b) { return b ? b->contact.tau_sim : nullptr; }
extern "C" double* saip_batch_contact_readout_device(saip_batch* b) { return b ? b->contact.readout : nullptr; }
extern "C" double* saip_batch_contact_summary_device(saip_batch* b) { return b ? b->contact.summary : nullptr; }
// one launch of the contact kernel at the resident state; dt: the substep an APPLY launch stands in front of
static saip_status contact_launch(saip_batch* b, int mode, double dt) {
	const auto& C = b->contact;
	{
		CycleParams cp;  // (the task constants on the device must be current: uploaded here when the configuration changed)
		saip_status st = make_params(b, cp, false);
		if (st) return st;
	}
	saip::ContactParams P;
	memset(&P, 0, sizeof(P));
	P.B = b->B;
	P.ld = b->ld;
	P.n = b->model->n;
	P.mode = mode;
	P.task = C.task;
	P.n_planes = C.n_planes;
	P.per_instance = C.per_instance;
	P.dt = dt;
	for (int e = 0; e < 3; e++) P.rc[e] = C.rc[e];
	P.model = b->model_dev;
	P.tasks = b->tasks_dev;
	P.q = b->q;
	P.dq = b->dq;
	P.planes = C.planes;
	P.goal = b->tasks[C.task].goal_dev;
	P.tau_cmd = b->plant.attached ? b->plant.tau_act : b->tau_bound ? b->tau_bound : b->tau;  // (read by APPLY only, which follows the plant launch)
	P.tau_sim = C.tau_sim;
	P.readout = C.readout;
	P.summary = C.summary;
	hipError_t e = saip::launch_contact_apply(P, b->model->dev.is_tree != 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "contact launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_contact_sense(saip_batch* b) {
	const char* fn = "saip_batch_contact_sense";
	saip_status st = need_contact(b, fn);
	if (st) return st;
	if (!b->contact.sensor) return fail(SAIP_ERR_ORDER, "%s: the contact planes were attached without the simulated sensor", fn);
	if ((st = need_ready(b, fn))) return st;
	return contact_launch(b, saip::CONTACT_SENSE, 0.0);
}
extern "C" saip_status saip_batch_contact_readout_host(saip_batch* b, double* out) {
	const char* fn = "saip_batch_contact_readout_host";
	saip_status st = need_contact(b, fn);
	if (st) return st;
	if (!out) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null output", fn);
	if ((st = need_ready(b, fn))) return st;
	return copy_d2h(b, out, b->contact.readout, saip::CONTACT_READOUT_ROWS);
}
extern "C" saip_status saip_batch_contact_summary_host(saip_batch* b, double* out) {
	const char* fn = "saip_batch_contact_summary_host";
	saip_status st = need_contact(b, fn);
	if (st) return st;
	if (!out) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null output", fn);
	if ((st = need_ready(b, fn))) return st;
	return copy_d2h(b, out, b->contact.summary, saip::CONTACT_SUMMARY_ROWS);
}
extern "C" saip_status saip_batch_contact_summary_reset(saip_batch* b) {
	const char* fn = "saip_batch_contact_summary_reset";
	saip_status st = need_contact(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	HIP_TRY(hipMemsetAsync(b->contact.summary, 0, (size_t)saip::CONTACT_SUMMARY_ROWS * b->ld * sizeof(double), b->stream));
	return SAIP_OK;
}

// ---- contact patches (saip_contact_patch.hip): up to eight points per patch, net force and moment, up to two patches on different tasks
// the slot of the patch on `task` (-1: of the first patch); < 0 with the error set
static int patch_slot(const saip_batch* b, int task, const char* fn, saip_status* st) {
	if ((*st = need_controller(b, fn))) return -1;
	if (b->n_patch == 0) {
		*st = fail(SAIP_ERR_ORDER, "%s: no contact patch is attached (saip_batch_contact_patch_attach)", fn);
		return -1;
	}
	if (task == -1) return 0;
	for (int i = 0; i < b->n_patch; i++)
		if (b->patch[i].task == task) return i;
	*st = fail(SAIP_ERR_ORDER, "%s: task %d carries no contact patch", fn, task);
	return -1;
}
static void patch_free(saip_batch* b, int slot) {
	auto& C = b->patch[slot];
	for (void* p : {(void*)C.planes, (void*)C.readout, (void*)C.summary})
		if (p) (void)hipFree(p);
	for (int i = slot; i + 1 < b->n_patch; i++) b->patch[i] = b->patch[i + 1];
	b->patch[b->n_patch - 1] = saip_batch::ContactPatch();
	if (--b->n_patch == 0 && b->patch_tau_sim) {
		(void)hipFree(b->patch_tau_sim);
		b->patch_tau_sim = nullptr;
	}
}
extern "C" saip_status saip_batch_contact_patch_attach(saip_batch* b, int task, int n_points, const double* points, int n_planes, const double* planes,
													   int per_instance, int sensor) {
	const char* fn = "saip_batch_contact_patch_attach";
	saip_status st = need_controller(b, fn);
	if (st || (st = contact_attach_task(b, task, fn))) return st;
	if (b->contact.attached) return fail(SAIP_ERR_ORDER, "%s: single-point contact planes are attached (saip_batch_contact_detach first)", fn);
	if (b->n_patch == saip::PATCH_MAX) return fail(SAIP_ERR_ORDER, "%s: %d contact patches are attached already", fn, saip::PATCH_MAX);
	for (int i = 0; i < b->n_patch; i++)
		if (b->patch[i].task == task) return fail(SAIP_ERR_ORDER, "%s: task %d already carries a contact patch (saip_batch_contact_patch_detach first)", fn, task);
	per_instance = per_instance ? 1 : 0;
	sensor = sensor ? 1 : 0;
	if (n_points < 1 || n_points > saip::PATCH_MAX_POINTS) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: 1..%d points required (got %d)", fn, saip::PATCH_MAX_POINTS, n_points);
	if (!points) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null points", fn);
	for (int i = 0; i < 3 * n_points; i++)
		if (!std::isfinite(points[i])) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: a contact point is not finite", fn);
	std::vector<double> host;
	if ((st = contact_attach_planes(b, task, n_planes, planes, per_instance, sensor, host, fn)) || (st = need_ready(b, fn))) return st;
	const size_t ld = b->ld, rows = (size_t)n_planes * saip::CONTACT_PLANE_WORDS;
	if (!b->patch_tau_sim && (st = contact_alloc_zero(b, &b->patch_tau_sim, (size_t)b->model->n * ld))) return st;
	const int slot = b->n_patch++;
	auto& C = b->patch[slot];
	if ((st = contact_alloc_zero(b, &C.planes, rows * (per_instance ? ld : 1))) || (st = contact_alloc_zero(b, &C.readout, (size_t)saip::PATCH_READOUT_ROWS * ld)) ||
		(st = contact_alloc_zero(b, &C.summary, (size_t)saip::PATCH_SUMMARY_ROWS * ld)) || (st = contact_upload_planes(b, C.planes, host, n_planes, per_instance, fn))) {
		patch_free(b, slot);
		return st;
	}
	C.task = task;
	C.n_points = n_points;
	C.n_planes = n_planes;
	C.per_instance = per_instance;
	C.sensor = sensor;
	for (int i = 0; i < 3 * n_points; i++) C.r[i / 3][i % 3] = points[i];
	b->otg_prelaunched = false;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_contact_patch_detach(saip_batch* b, int task) {
	const char* fn = "saip_batch_contact_patch_detach";
	saip_status st;
	const int slot = patch_slot(b, task, fn, &st);
	if (slot < 0 || (st = need_ready(b, fn))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));  // a contact substep may still be in flight
	if (task == -1)
		while (b->n_patch > 0) patch_free(b, b->n_patch - 1);
	else patch_free(b, slot);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_contact_patch_info(saip_batch* b, int task, int* n_patches, int* n_points, int* n_planes, int* per_instance, int* sensor,
													 double* points) {
	saip_status st;
	const int slot = patch_slot(b, task, "saip_batch_contact_patch_info", &st);
	if (slot < 0) return st;
	const auto& C = b->patch[slot];
	if (n_patches) *n_patches = b->n_patch;
	if (n_points) *n_points = C.n_points;
	if (n_planes) *n_planes = C.n_planes;
	if (per_instance) *per_instance = C.per_instance;
	if (sensor) *sensor = C.sensor;
	for (int i = 0; i < 3 * C.n_points && points; i++) points[i] = C.r[i / 3][i % 3];
	return SAIP_OK;
}
extern "C" saip_status saip_batch_contact_patch_set_planes_host(saip_batch* b, int task, const double* planes) {
	const char* fn = "saip_batch_contact_patch_set_planes_host";
	saip_status st;
	const int slot = patch_slot(b, task, fn, &st);
	if (slot < 0) return st;
	if (!planes) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null planes", fn);
	const auto& C = b->patch[slot];
	std::vector<double> host;
	if (const char* bad = contact_check_planes(planes, C.n_planes, C.per_instance ? (size_t)b->B : 1, host)) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, bad);
	if ((st = need_ready(b, fn))) return st;
	return contact_upload_planes(b, C.planes, host, C.n_planes, C.per_instance, fn);
}
static const saip_batch::ContactPatch* patch_of(const saip_batch* b, int task) {
	if (!b) return nullptr;
	for (int i = 0; i < b->n_patch; i++)
		if (b->patch[i].task == task || task == -1) return &b->patch[i];
	return nullptr;
}
extern "C" double* saip_batch_contact_patch_planes_device(saip_batch* b, int task) { return patch_of(b, task) ? patch_of(b, task)->planes : nullptr; }
extern "C" double* saip_batch_contact_patch_readout_device(saip_batch* b, int task) { return patch_of(b, task) ? patch_of(b, task)->readout : nullptr; }
extern "C" double* saip_batch_contact_patch_summary_device(saip_batch* b, int task) { return patch_of(b, task) ? patch_of(b, task)->summary : nullptr; }
extern "C" double* saip_batch_contact_patch_torques_device(saip_batch* b) { return b ? b->patch_tau_sim : nullptr; }
// one launch of the patch kernel at the resident state, for every patch; dt: the substep an APPLY launch stands in front of
static saip_status patch_launch(saip_batch* b, int mode, double dt) {
	{
		CycleParams cp;  // (the task constants on the device must be current: uploaded here when the configuration changed)
		saip_status st = make_params(b, cp, false);
		if (st) return st;
	}
	saip::ContactPatchParams P;
	memset(&P, 0, sizeof(P));
	P.B = b->B;
	P.ld = b->ld;
	P.n = b->model->n;
	P.mode = mode;
	P.n_patches = b->n_patch;
	P.dt = dt;
	P.model = b->model_dev;
	P.tasks = b->tasks_dev;
	P.q = b->q;
	P.dq = b->dq;
	P.tau_cmd = b->plant.attached ? b->plant.tau_act : b->tau_bound ? b->tau_bound : b->tau;  // (read by APPLY only, which follows the plant launch)
	P.tau_sim = b->patch_tau_sim;
	for (int i = 0; i < b->n_patch; i++) {
		const auto& C = b->patch[i];
		saip::PatchDev& D = P.patch[i];
		D.task = C.task;
		D.n_points = C.n_points;
		D.n_planes = C.n_planes;
		D.per_instance = C.per_instance;
		D.sensor = C.sensor;
		memcpy(D.r, C.r, sizeof(D.r));
		D.planes = C.planes;
		D.goal = b->tasks[C.task].goal_dev;
		D.readout = C.readout;
		D.summary = C.summary;
	}
	hipError_t e = saip::launch_contact_patch_apply(P, b->model->dev.is_tree != 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "contact patch launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}
static bool patch_any_sensor(const saip_batch* b) {
	for (int i = 0; i < b->n_patch; i++)
		if (b->patch[i].sensor) return true;
	return false;
}
extern "C" saip_status saip_batch_contact_patch_sense(saip_batch* b) {
	const char* fn = "saip_batch_contact_patch_sense";
	saip_status st;
	if (patch_slot(b, -1, fn, &st) < 0) return st;
	if (!patch_any_sensor(b)) return fail(SAIP_ERR_ORDER, "%s: no contact patch was attached with the simulated sensor", fn);
	if ((st = need_ready(b, fn))) return st;
	return patch_launch(b, saip::CONTACT_SENSE, 0.0);
}
extern "C" saip_status saip_batch_contact_patch_readout_host(saip_batch* b, int task, double* out) {
	const char* fn = "saip_batch_contact_patch_readout_host";
	saip_status st;
	const int slot = patch_slot(b, task, fn, &st);
	if (slot < 0) return st;
	if (!out) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null output", fn);
	if ((st = need_ready(b, fn))) return st;
	return copy_d2h(b, out, b->patch[slot].readout, saip::PATCH_READOUT_ROWS);
}
extern "C" saip_status saip_batch_contact_patch_summary_host(saip_batch* b, int task, double* out) {
	const char* fn = "saip_batch_contact_patch_summary_host";
	saip_status st;
	const int slot = patch_slot(b, task, fn, &st);
	if (slot < 0) return st;
	if (!out) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null output", fn);
	if ((st = need_ready(b, fn))) return st;
	return copy_d2h(b, out, b->patch[slot].summary, saip::PATCH_SUMMARY_ROWS);
}
extern "C" saip_status saip_batch_contact_patch_summary_reset(saip_batch* b, int task) {
	const char* fn = "saip_batch_contact_patch_summary_reset";
	saip_status st;
	const int slot = patch_slot(b, task, fn, &st);
	if (slot < 0 || (st = need_ready(b, fn))) return st;
	for (int i = 0; i < b->n_patch; i++)
		if (task == -1 || i == slot) HIP_TRY(hipMemsetAsync(b->patch[i].summary, 0, (size_t)saip::PATCH_SUMMARY_ROWS * b->ld * sizeof(double), b->stream));
	return SAIP_OK;
}

// ---- the clearance monitor (saip_clearance.hip): link spheres against world-fixed obstacles and against each other
static saip_status need_clearance(const saip_batch* b, const char* fn) {
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!b->clearance.attached) return fail(SAIP_ERR_ORDER, "%s: no clearance monitor is attached (saip_batch_clearance_attach)", fn);
	return SAIP_OK;
}
static void clearance_free(saip_batch* b) {
	auto& C = b->clearance;
	for (void* p : {(void*)C.geom_dev, (void*)C.obst, (void*)C.readout, (void*)C.summary, (void*)C.centres})
		if (p) (void)hipFree(p);
	C = saip_batch::Clearance();
}
// the obstacle table [O][8] or [O][8][B]; false: `msg` says what is wrong with which entry
static bool clearance_check_obstacles(const double* obst, int O, size_t cols, char* msg, size_t len) {
	for (int o = 0; o < O; o++)
		for (size_t i = 0; i < cols; i++) {
			const double* w = obst + (size_t)o * saip::CLEARANCE_OBSTACLE_WORDS * cols + i;
			char where[48] = "";
			if (cols > 1) snprintf(where, sizeof(where), " of instance %zu", i);
			for (int k = 0; k < saip::CLEARANCE_OBSTACLE_WORDS; k++)
				if (!std::isfinite(w[k * cols])) return snprintf(msg, len, "obstacle %d%s: word %d is not finite", o, where, k), false;
			if (w[0] == (double)saip::CLEARANCE_CAPSULE) {
				if (w[7 * cols] < 0) return snprintf(msg, len, "obstacle %d%s: radius %g below 0", o, where, w[7 * cols]), false;
			} else if (w[0] == (double)saip::CLEARANCE_HALF_SPACE) {
				const double nn = std::sqrt(w[cols] * w[cols] + w[2 * cols] * w[2 * cols] + w[3 * cols] * w[3 * cols]);
				if (!(std::fabs(nn - 1.0) <= 1e-6)) return snprintf(msg, len, "obstacle %d%s: the half-space normal has length %.9g, not 1", o, where, nn), false;
			} else {
				return snprintf(msg, len, "obstacle %d%s: unknown kind %g (0 capsule, 1 half-space)", o, where, w[0]), false;
			}
		}
	return true;
}
static saip_status clearance_upload_obstacles(saip_batch* b, double* dev, const double* host, int O, int per_instance, const char* fn) {
	if (O == 0) return SAIP_OK;
	const size_t rows = (size_t)O * saip::CLEARANCE_OBSTACLE_WORDS;
	hipError_t e;
	if (per_instance)
		e = hipMemcpy2DAsync(dev, (size_t)b->ld * sizeof(double), host, (size_t)b->B * sizeof(double), (size_t)b->B * sizeof(double), rows,
							 hipMemcpyHostToDevice, b->stream);
	else e = hipMemcpyAsync(dev, host, rows * sizeof(double), hipMemcpyHostToDevice, b->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(b->stream);  // the caller may reuse `host` right away
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "%s: obstacle upload failed: %s", fn, hipGetErrorString(e));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_clearance_attach(saip_batch* b, int n_spheres, const int* links, const double* centres, const double* radii,
												   int n_obstacles, const double* obstacles, int per_instance, int n_pairs, const int* pairs, double margin,
												   int keep_centres) {
	const char* fn = "saip_batch_clearance_attach";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (b->clearance.attached) return fail(SAIP_ERR_ORDER, "%s: a clearance monitor is already attached (saip_batch_clearance_detach first)", fn);
	const int S = n_spheres, O = n_obstacles, NP = n_pairs;
	if (S < 1 || S > saip::CLEARANCE_MAX_SPHERES) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: 1..%d spheres required (got %d)", fn, saip::CLEARANCE_MAX_SPHERES, S);
	if (O < 0 || O > saip::CLEARANCE_MAX_OBSTACLES) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: 0..%d obstacles required (got %d)", fn, saip::CLEARANCE_MAX_OBSTACLES, O);
	if (NP < 0 || NP > saip::CLEARANCE_MAX_PAIRS) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: 0..%d pairs required (got %d)", fn, saip::CLEARANCE_MAX_PAIRS, NP);
	if (O == 0 && NP == 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: nothing to measure against: 0 obstacles and 0 pairs", fn);
	if (!links || !centres || !radii) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null links, centres or radii", fn);
	if (O > 0 && !obstacles) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null obstacles", fn);
	if (NP > 0 && !pairs) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null pairs", fn);
	if (!(margin >= 0) || !std::isfinite(margin)) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: margin %g is negative or not finite", fn, margin);
	per_instance = per_instance ? 1 : 0;
	keep_centres = keep_centres ? 1 : 0;
	const int nl = (int)b->model->links.size();
	for (int s = 0; s < S; s++) {
		if (links[s] < 0 || links[s] >= nl) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: sphere %d: link index %d out of range (%d links)", fn, s, links[s], nl);
		for (int e = 0; e < 3; e++)
			if (!std::isfinite(centres[3 * s + e])) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: sphere %d: the centre is not finite", fn, s);
		if (!std::isfinite(radii[s])) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: sphere %d: the radius is not finite", fn, s);
		if (radii[s] < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: sphere %d: radius %g below 0", fn, s, radii[s]);
	}
	for (int p = 0; p < NP; p++) {
		const int s1 = pairs[2 * p], s2 = pairs[2 * p + 1];
		if (s1 < 0 || s1 >= S || s2 < 0 || s2 >= S) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: pair %d: sphere index (%d, %d) out of range (%d spheres)", fn, p, s1, s2, S);
		if (s1 == s2) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: pair %d: sphere %d against itself", fn, p, s1);
	}
	char msg[160];
	if (!clearance_check_obstacles(obstacles, O, per_instance ? (size_t)b->B : 1, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	// [O][8][ld], [3 S][ld] doubles: the byte counts must fit a size_t
	const size_t widest = (size_t)saip::CLEARANCE_MAX_OBSTACLES * saip::CLEARANCE_OBSTACLE_WORDS * sizeof(double);
	if ((size_t)b->ld > SIZE_MAX / widest) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: arrays of leading dimension %d are too large", fn, b->ld);
	if ((st = need_ready(b, fn))) return st;
	auto& C = b->clearance;
	C = saip_batch::Clearance();
	saip::ClearanceGeom& G = C.geom;
	memset(&G, 0, sizeof(G));
	G.S = S;
	G.O = O;
	G.P = NP;
	// the spheres sorted by body (stable), their constants composed exactly as saip_batch_model_frames_* composes a frame's point, so that a
	// centre differs from that query's position by the contraction of the walk alone
	int order[saip::CLEARANCE_MAX_SPHERES];
	for (int s = 0; s < S; s++) order[s] = s;
	for (int i = 1; i < S; i++)
		for (int k = i; k > 0 && b->model->links[links[order[k - 1]]].body > b->model->links[links[order[k]]].body; k--) std::swap(order[k - 1], order[k]);
	for (int i = 0; i < S; i++) {
		const int s = order[i];
		const LinkInfo& L = b->model->links[links[s]];
		double t[3];
		m3_vec(L.R, centres + 3 * s, t);
		for (int e = 0; e < 3; e++) G.r[i][e] = L.p[e] + t[e];
		G.body[i] = L.body;
		G.slot[i] = s;
		G.radius[s] = radii[s];
	}
	for (int p = 0; p < NP; p++) {
		G.pair[p][0] = (uint8_t)pairs[2 * p];
		G.pair[p][1] = (uint8_t)pairs[2 * p + 1];
	}
	auto alloc_zero = [&](double** p, size_t count) -> saip_status {
		HIP_TRY(hipMalloc((void**)p, count * sizeof(double)));
		HIP_TRY(hipMemsetAsync(*p, 0, count * sizeof(double), b->stream));
		return SAIP_OK;
	};
	auto upload_geom = [&]() -> saip_status {
		HIP_TRY(hipMalloc((void**)&C.geom_dev, sizeof(G)));
		HIP_TRY(hipMemcpyAsync(C.geom_dev, &G, sizeof(G), hipMemcpyHostToDevice, b->stream));
		HIP_TRY(hipStreamSynchronize(b->stream));
		return SAIP_OK;
	};
	auto reset = [&]() -> saip_status {
		HIP_TRY(saip::launch_clearance_summary_reset(b->B, b->ld, C.summary, b->stream));
		return SAIP_OK;
	};
	const size_t ld = b->ld, rows = (size_t)O * saip::CLEARANCE_OBSTACLE_WORDS;
	if ((st = upload_geom()) || (O > 0 && (st = alloc_zero(&C.obst, rows * (per_instance ? ld : 1)))) ||
		(st = alloc_zero(&C.readout, (size_t)saip::CLEARANCE_READOUT_ROWS * ld)) || (st = alloc_zero(&C.summary, (size_t)saip::CLEARANCE_SUMMARY_ROWS * ld)) ||
		(keep_centres && (st = alloc_zero(&C.centres, (size_t)3 * S * ld))) || (st = clearance_upload_obstacles(b, C.obst, obstacles, O, per_instance, fn)) ||
		(st = reset())) {
		clearance_free(b);
		return st;
	}
	C.attached = true;
	C.per_instance = per_instance;
	C.keep_centres = keep_centres;
	C.margin = margin;
	C.period = 0;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_clearance_detach(saip_batch* b) {
	const char* fn = "saip_batch_clearance_detach";
	saip_status st = need_clearance(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));  // a launch may still be in flight
	clearance_free(b);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_clearance_info(saip_batch* b, int* n_spheres, int* n_obstacles, int* per_instance, int* n_pairs, double* margin,
												 int* keep_centres, long long* period) {
	saip_status st = need_clearance(b, "saip_batch_clearance_info");
	if (st) return st;
	const auto& C = b->clearance;
	if (n_spheres) *n_spheres = C.geom.S;
	if (n_obstacles) *n_obstacles = C.geom.O;
	if (per_instance) *per_instance = C.per_instance;
	if (n_pairs) *n_pairs = C.geom.P;
	if (margin) *margin = C.margin;
	if (keep_centres) *keep_centres = C.keep_centres;
	if (period) *period = C.period;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_clearance_set_obstacles_host(saip_batch* b, const double* obstacles) {
	const char* fn = "saip_batch_clearance_set_obstacles_host";
	saip_status st = need_clearance(b, fn);
	if (st) return st;
	const auto& C = b->clearance;
	if (C.geom.O == 0) return fail(SAIP_ERR_ORDER, "%s: the monitor was attached without obstacles", fn);
	if (!obstacles) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null obstacles", fn);
	char msg[160];
	if (!clearance_check_obstacles(obstacles, C.geom.O, C.per_instance ? (size_t)b->B : 1, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	if ((st = need_ready(b, fn))) return st;
	return clearance_upload_obstacles(b, C.obst, obstacles, C.geom.O, C.per_instance, fn);
}
extern "C" double* saip_batch_clearance_obstacles_device(saip_batch* b) { return b ? b->clearance.obst : nullptr; }
extern "C" double* saip_batch_clearance_readout_device(saip_batch* b) { return b ? b->clearance.readout : nullptr; }
extern "C" double* saip_batch_clearance_summary_device(saip_batch* b) { return b ? b->clearance.summary : nullptr; }
extern "C" double* saip_batch_clearance_centres_device(saip_batch* b) { return b ? b->clearance.centres : nullptr; }
// one launch of the clearance kernel at the resident state; MONITOR takes the next period index from the host counter (as the goal schedules do)
static saip_status clearance_launch(saip_batch* b, int mode, double dt) {
	auto& C = b->clearance;
	saip::ClearanceParams P;
	memset(&P, 0, sizeof(P));
	P.B = b->B;
	P.ld = b->ld;
	P.n = b->model->n;
	P.mode = mode;
	P.per_instance = C.per_instance;
	P.dt = dt;
	P.period = mode == saip::CLEARANCE_MONITOR ? (double)C.period++ : 0.0;
	P.margin = C.margin;
	P.model = b->model_dev;
	P.geom = C.geom_dev;
	P.q = b->q;
	P.obst = C.obst;
	P.readout = C.readout;
	P.summary = C.summary;
	P.centres = C.centres;
	hipError_t e = saip::launch_clearance_eval(P, b->model->dev.is_tree != 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "clearance launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_clearance_evaluate(saip_batch* b) {
	const char* fn = "saip_batch_clearance_evaluate";
	saip_status st = need_clearance(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	return clearance_launch(b, saip::CLEARANCE_EVALUATE, 0.0);
}
extern "C" saip_status saip_batch_clearance_readout_host(saip_batch* b, double* out) {
	const char* fn = "saip_batch_clearance_readout_host";
	saip_status st = need_clearance(b, fn);
	if (st) return st;
	if (!out) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null output", fn);
	if ((st = need_ready(b, fn))) return st;
	return copy_d2h(b, out, b->clearance.readout, saip::CLEARANCE_READOUT_ROWS);
}
extern "C" saip_status saip_batch_clearance_summary_host(saip_batch* b, double* out) {
	const char* fn = "saip_batch_clearance_summary_host";
	saip_status st = need_clearance(b, fn);
	if (st) return st;
	if (!out) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null output", fn);
	if ((st = need_ready(b, fn))) return st;
	return copy_d2h(b, out, b->clearance.summary, saip::CLEARANCE_SUMMARY_ROWS);
}
// row 0 to +inf, row 3 to -1 (a memset cannot), the period counter to 0
extern "C" saip_status saip_batch_clearance_summary_reset(saip_batch* b) {
	const char* fn = "saip_batch_clearance_summary_reset";
	saip_status st = need_clearance(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	HIP_TRY(saip::launch_clearance_summary_reset(b->B, b->ld, b->clearance.summary, b->stream));
	b->clearance.period = 0;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_clearance_add_cost(saip_batch* b, double w_penalty, double w_collision, double d_safe) {
	const char* fn = "saip_batch_clearance_add_cost";
	saip_status st = need_clearance(b, fn);
	if (st) return st;
	if (b->n_samp == 0) return fail(SAIP_ERR_ORDER, "%s: no sampler is attached (saip_batch_sampler_attach): there is no cost to add to", fn);
	if (w_penalty != w_penalty || w_collision != w_collision || d_safe != d_safe) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: a weight or d_safe is NaN", fn);
	if ((st = need_ready(b, fn))) return st;
	HIP_TRY(saip::launch_clearance_add_cost(b->B, b->ld, b->clearance.summary, b->samp_cost, w_penalty, w_collision, d_safe, b->stream));
	return SAIP_OK;
}

// ---- the plant model (saip_plant.hip): actuator limits, friction, joint stops and external wrenches in front of every integration substep
static saip_status need_plant(const saip_batch* b, const char* fn) {
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!b->plant.attached) return fail(SAIP_ERR_ORDER, "%s: no plant model is attached (saip_batch_plant_attach)", fn);
	return SAIP_OK;
}
static void plant_free(saip_batch* b) {
	auto& C = b->plant;
	for (void* p : {(void*)C.joints, (void*)C.wrenches, (void*)C.tau_act, (void*)C.summary, (void*)C.bounds})
		if (p) (void)hipFree(p);
	C = saip_batch::Plant();
}
static const char* const PLANT_JOINT_WORD_NAMES[saip::PLANT_JOINT_WORDS] = {"gain", "bias", "tau_max", "fv", "fc", "v_s", "q_lo", "q_hi", "k_stop", "c_stop"};
static const char* const PLANT_WRENCH_WORD_NAMES[saip::PLANT_WRENCH_WORDS] = {"F[0]", "F[1]", "F[2]", "M[0]", "M[1]", "M[2]", "p_start", "p_end"};
// a joint table [n][10] (cols = 1) or [n][10][cols]: true when fine, else msg names the joint and the word (and the instance)
static bool plant_check_joints(const double* t, int n, size_t cols, char* msg, size_t len) {
	using namespace saip;
	for (int j = 0; j < n; j++)
		for (size_t i = 0; i < cols; i++) {
			const double* w = t + (size_t)j * PLANT_JOINT_WORDS * cols + i;
			char who[64];
			if (cols > 1) snprintf(who, sizeof(who), "joint %d of instance %zu", j, i);
			else snprintf(who, sizeof(who), "joint %d", j);
			for (int k = 0; k < PLANT_JOINT_WORDS; k++) {
				const double v = w[k * cols];
				if (v != v) return snprintf(msg, len, "%s: word %s is NaN", who, PLANT_JOINT_WORD_NAMES[k]), false;
				const bool may_be_infinite = k == PLANT_TAU_MAX || k == PLANT_VS || k == PLANT_Q_LO || k == PLANT_Q_HI;
				if (!may_be_infinite && !std::isfinite(v)) return snprintf(msg, len, "%s: word %s is not finite", who, PLANT_JOINT_WORD_NAMES[k]), false;
				const bool not_negative = k == PLANT_TAU_MAX || k == PLANT_FV || k == PLANT_FC || k == PLANT_K_STOP || k == PLANT_C_STOP;
				if (not_negative && v < 0) return snprintf(msg, len, "%s: word %s = %g is below 0", who, PLANT_JOINT_WORD_NAMES[k], v), false;
			}
			if (w[PLANT_FC * cols] > 0 && !(w[PLANT_VS * cols] > 0)) return snprintf(msg, len, "%s: word v_s = %g must be positive when fc > 0", who, w[PLANT_VS * cols]), false;
			if (w[PLANT_Q_LO * cols] > w[PLANT_Q_HI * cols])
				return snprintf(msg, len, "%s: word q_lo = %g is above q_hi = %g", who, w[PLANT_Q_LO * cols], w[PLANT_Q_HI * cols]), false;
		}
	return true;
}
// a wrench table [W][8] or [W][8][cols]: F and M finite, the window words anything but NaN
static bool plant_check_wrenches(const double* t, int W, size_t cols, char* msg, size_t len) {
	for (int k = 0; k < W; k++)
		for (size_t i = 0; i < cols; i++)
			for (int e = 0; e < saip::PLANT_WRENCH_WORDS; e++) {
				const double v = t[((size_t)k * saip::PLANT_WRENCH_WORDS + e) * cols + i];
				if (v != v || (e < 6 && !std::isfinite(v))) {
					if (cols > 1) snprintf(msg, len, "wrench %d of instance %zu: word %s is not finite", k, i, PLANT_WRENCH_WORD_NAMES[e]);
					else snprintf(msg, len, "wrench %d: word %s is not finite", k, PLANT_WRENCH_WORD_NAMES[e]);
					return false;
				}
			}
	return true;
}
// host [rows] or [rows][B] -> device [rows] or [rows][ld]
static saip_status plant_upload(saip_batch* b, double* dev, const double* host, size_t rows, int per_instance, const char* fn) {
	hipError_t e;
	if (per_instance)
		e = hipMemcpy2DAsync(dev, (size_t)b->ld * sizeof(double), host, (size_t)b->B * sizeof(double), (size_t)b->B * sizeof(double), rows, hipMemcpyHostToDevice,
							 b->stream);
	else e = hipMemcpyAsync(dev, host, rows * sizeof(double), hipMemcpyHostToDevice, b->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(b->stream);  // the host buffer may be reused by the caller right away
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "%s: table upload failed: %s", fn, hipGetErrorString(e));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_plant_attach(saip_batch* b, const double* joint_table, int per_instance_joints, int n_wrenches, const int* links,
												const double* points, const int* frames, const double* wrench_table, int per_instance_wrenches) {
	const char* fn = "saip_batch_plant_attach";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (b->plant.attached) return fail(SAIP_ERR_ORDER, "%s: a plant model is already attached (saip_batch_plant_detach first)", fn);
	const int W = n_wrenches, n = b->model->n;
	if (W < 0 || W > saip::PLANT_MAX_WRENCHES) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: 0..%d wrenches required (got %d)", fn, saip::PLANT_MAX_WRENCHES, W);
	if (W > 0 && (!links || !points || !frames || !wrench_table)) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null links, points, frames or wrench table", fn);
	per_instance_joints = per_instance_joints ? 1 : 0;
	per_instance_wrenches = per_instance_wrenches && W > 0 ? 1 : 0;
	saip::PlantSite site[saip::PLANT_MAX_WRENCHES] = {};
	const int nl = (int)b->model->links.size();
	double I3[9];
	m3_eye(I3);
	for (int k = 0; k < W; k++) {
		if (links[k] < 0 || links[k] >= nl) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: wrench %d: link index %d out of range (%d links)", fn, k, links[k], nl);
		for (int e = 0; e < 3; e++)
			if (!std::isfinite(points[3 * k + e])) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: wrench %d: the point is not finite", fn, k);
		if (frames[k] != saip::PLANT_FRAME_WORLD && frames[k] != saip::PLANT_FRAME_LINK)
			return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: wrench %d: unknown frame %d (0 world, 1 link)", fn, k, frames[k]);
		// the site composed exactly as saip_batch_model_frames_* composes a frame's point and rotation
		const LinkInfo& L = b->model->links[links[k]];
		double t[3];
		m3_vec(L.R, points + 3 * k, t);
		for (int e = 0; e < 3; e++) site[k].pos[e] = L.p[e] + t[e];
		m3_mul(L.R, I3, site[k].rot);
		site[k].body = L.body;
		site[k].frame = frames[k];
	}
	// the neutral table: gain 1, no offset, no limit, no friction, the model's joint limits as stops of stiffness 0
	const size_t jcols = per_instance_joints ? (size_t)b->B : 1, wcols = per_instance_wrenches ? (size_t)b->B : 1;
	std::vector<double> neutral;
	if (!joint_table) {
		neutral.assign((size_t)n * saip::PLANT_JOINT_WORDS * jcols, 0.0);
		for (int j = 0; j < n; j++) {
			const double lo = b->model->q_lower[j], hi = b->model->q_upper[j];
			const bool limits = lo <= hi;
			for (size_t i = 0; i < jcols; i++) {
				double* w = neutral.data() + (size_t)j * saip::PLANT_JOINT_WORDS * jcols + i;
				w[saip::PLANT_GAIN * jcols] = 1.0;
				w[saip::PLANT_TAU_MAX * jcols] = INFINITY;
				w[saip::PLANT_Q_LO * jcols] = limits ? lo : -INFINITY;
				w[saip::PLANT_Q_HI * jcols] = limits ? hi : INFINITY;
			}
		}
		joint_table = neutral.data();
	}
	char msg[200];
	if (!plant_check_joints(joint_table, n, jcols, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	if (W > 0 && !plant_check_wrenches(wrench_table, W, wcols, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	// [n][10][ld] doubles: the byte count must fit a size_t
	const size_t widest = (size_t)(n > 4 ? n : 4) * saip::PLANT_JOINT_WORDS * sizeof(double);
	if ((size_t)b->ld > SIZE_MAX / widest) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: arrays of leading dimension %d are too large", fn, b->ld);
	if ((st = need_ready(b, fn))) return st;
	auto& C = b->plant;
	C = saip_batch::Plant();
	const size_t ld = b->ld, jrows = (size_t)n * saip::PLANT_JOINT_WORDS, wrows = (size_t)W * saip::PLANT_WRENCH_WORDS;
	if ((st = contact_alloc_zero(b, &C.joints, jrows * (per_instance_joints ? ld : 1))) || (W > 0 && (st = contact_alloc_zero(b, &C.wrenches, wrows * (per_instance_wrenches ? ld : 1)))) ||
		(st = contact_alloc_zero(b, &C.tau_act, (size_t)n * ld)) || (st = contact_alloc_zero(b, &C.summary, (size_t)saip::PLANT_SUMMARY_ROWS * ld)) ||
		((per_instance_joints || per_instance_wrenches) && (st = contact_alloc_zero(b, &C.bounds, 2 * (jrows + wrows)))) ||
		(st = plant_upload(b, C.joints, joint_table, jrows, per_instance_joints, fn)) ||
		(W > 0 && (st = plant_upload(b, C.wrenches, wrench_table, wrows, per_instance_wrenches, fn)))) {
		plant_free(b);
		return st;
	}
	C.attached = true;
	C.per_instance_joints = per_instance_joints;
	C.n_wrenches = W;
	C.per_instance_wrenches = per_instance_wrenches;
	C.period = 0;
	for (int k = 0; k < W; k++) C.site[k] = site[k];
	b->otg_prelaunched = false;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_plant_detach(saip_batch* b) {
	const char* fn = "saip_batch_plant_detach";
	saip_status st = need_plant(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));  // a plant substep may still be in flight
	plant_free(b);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_plant_info(saip_batch* b, int* per_instance_joints, int* n_wrenches, int* per_instance_wrenches, long long* period) {
	saip_status st = need_plant(b, "saip_batch_plant_info");
	if (st) return st;
	const auto& C = b->plant;
	if (per_instance_joints) *per_instance_joints = C.per_instance_joints;
	if (n_wrenches) *n_wrenches = C.n_wrenches;
	if (per_instance_wrenches) *per_instance_wrenches = C.per_instance_wrenches;
	if (period) *period = C.period;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_plant_set_joints_host(saip_batch* b, const double* joint_table) {
	const char* fn = "saip_batch_plant_set_joints_host";
	saip_status st = need_plant(b, fn);
	if (st) return st;
	if (!joint_table) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null joint table", fn);
	const auto& C = b->plant;
	char msg[200];
	if (!plant_check_joints(joint_table, b->model->n, C.per_instance_joints ? (size_t)b->B : 1, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	if ((st = need_ready(b, fn))) return st;
	return plant_upload(b, C.joints, joint_table, (size_t)b->model->n * saip::PLANT_JOINT_WORDS, C.per_instance_joints, fn);
}
extern "C" saip_status saip_batch_plant_set_wrenches_host(saip_batch* b, const double* wrench_table) {
	const char* fn = "saip_batch_plant_set_wrenches_host";
	saip_status st = need_plant(b, fn);
	if (st) return st;
	const auto& C = b->plant;
	if (C.n_wrenches == 0) return fail(SAIP_ERR_ORDER, "%s: the plant model was attached without wrenches", fn);
	if (!wrench_table) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null wrench table", fn);
	char msg[200];
	if (!plant_check_wrenches(wrench_table, C.n_wrenches, C.per_instance_wrenches ? (size_t)b->B : 1, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, msg);
	if ((st = need_ready(b, fn))) return st;
	return plant_upload(b, C.wrenches, wrench_table, (size_t)C.n_wrenches * saip::PLANT_WRENCH_WORDS, C.per_instance_wrenches, fn);
}
// Per-instance tables drawn on the device between two batch-uniform tables (host pointers: joints [n][10], wrenches [W][8]); a null pair
// leaves that table alone.  Whatever the draw, the tables stay valid: both bounds of every word have to be, and so has every combination
// the two-word conditions can meet (the largest q_lo against the smallest q_hi, the smallest v_s when fc can be positive).
extern "C" saip_status saip_batch_plant_randomize(saip_batch* b, unsigned long long seed, long long round, const double* joint_lo, const double* joint_hi,
												   const double* wrench_lo, const double* wrench_hi) {
	using namespace saip;
	const char* fn = "saip_batch_plant_randomize";
	saip_status st = need_plant(b, fn);
	if (st) return st;
	const auto& C = b->plant;
	const int n = b->model->n, W = C.n_wrenches;
	if ((joint_lo == nullptr) != (joint_hi == nullptr) || (wrench_lo == nullptr) != (wrench_hi == nullptr))
		return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: a lower table without its upper table (or the reverse)", fn);
	if (!joint_lo && !wrench_lo) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: nothing to draw: both pairs are null", fn);
	if (joint_lo && !C.per_instance_joints) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the joint table is batch-uniform (attach it per instance)", fn);
	if (wrench_lo && (W == 0 || !C.per_instance_wrenches)) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the wrench table is batch-uniform or empty (attach it per instance)", fn);
	char msg[200];
	const size_t jrows = (size_t)n * PLANT_JOINT_WORDS, wrows = (size_t)W * PLANT_WRENCH_WORDS;
	if (joint_lo) {
		for (const double* t : {joint_lo, joint_hi})
			if (!plant_check_joints(t, n, 1, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s bound: %s", fn, t == joint_lo ? "lower" : "upper", msg);
		for (int j = 0; j < n; j++) {
			const double *l = joint_lo + (size_t)j * PLANT_JOINT_WORDS, *h = joint_hi + (size_t)j * PLANT_JOINT_WORDS;
			for (int k = 0; k < PLANT_JOINT_WORDS; k++)
				if (l[k] != h[k] && !(std::isfinite(l[k]) && std::isfinite(h[k])))
					return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: joint %d: word %s has an infinite bound on one side only", fn, j, PLANT_JOINT_WORD_NAMES[k]);
			if (std::max(l[PLANT_Q_LO], h[PLANT_Q_LO]) > std::min(l[PLANT_Q_HI], h[PLANT_Q_HI]))
				return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: joint %d: the ranges of words q_lo and q_hi overlap", fn, j);
			if (std::max(l[PLANT_FC], h[PLANT_FC]) > 0 && !(std::min(l[PLANT_VS], h[PLANT_VS]) > 0))
				return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: joint %d: word v_s must be positive over its whole range when fc can be", fn, j);
		}
	}
	if (wrench_lo) {
		for (const double* t : {wrench_lo, wrench_hi})
			if (!plant_check_wrenches(t, W, 1, msg, sizeof(msg))) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s bound: %s", fn, t == wrench_lo ? "lower" : "upper", msg);
		for (size_t k = 0; k < wrows; k++)
			if (wrench_lo[k] != wrench_hi[k] && !(std::isfinite(wrench_lo[k]) && std::isfinite(wrench_hi[k])))
				return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: wrench %zu: word %s has an infinite bound on one side only", fn, k / PLANT_WRENCH_WORDS, PLANT_WRENCH_WORD_NAMES[k % PLANT_WRENCH_WORDS]);
	}
	if ((st = need_ready(b, fn))) return st;
	PlantRandomParams P;
	memset(&P, 0, sizeof(P));
	P.B = b->B;
	P.ld = b->ld;
	P.n = n;
	P.n_wrenches = W;
	P.seed_lo = (uint32_t)seed;
	P.seed_hi = (uint32_t)(seed >> 32);
	P.round = (uint32_t)round;
	double* jb = C.bounds;
	double* wb = C.bounds + 2 * jrows;
	if (joint_lo) {
		if ((st = plant_upload(b, jb, joint_lo, jrows, 0, fn)) || (st = plant_upload(b, jb + jrows, joint_hi, jrows, 0, fn))) return st;
		P.joints = C.joints;
		P.joint_lo = jb;
		P.joint_hi = jb + jrows;
	}
	if (wrench_lo) {
		if ((st = plant_upload(b, wb, wrench_lo, wrows, 0, fn)) || (st = plant_upload(b, wb + wrows, wrench_hi, wrows, 0, fn))) return st;
		P.wrenches = C.wrenches;
		P.wrench_lo = wb;
		P.wrench_hi = wb + wrows;
	}
	hipError_t e = saip::launch_plant_randomize(P, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "plant randomize launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_plant_set_period(saip_batch* b, long long period) {
	saip_status st = need_plant(b, "saip_batch_plant_set_period");
	if (st) return st;
	b->plant.period = period;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_plant_summary_host(saip_batch* b, double* out) {
	const char* fn = "saip_batch_plant_summary_host";
	saip_status st = need_plant(b, fn);
	if (st) return st;
	if (!out) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null output", fn);
	if ((st = need_ready(b, fn))) return st;
	return copy_d2h(b, out, b->plant.summary, saip::PLANT_SUMMARY_ROWS);
}
extern "C" saip_status saip_batch_plant_summary_reset(saip_batch* b) {
	const char* fn = "saip_batch_plant_summary_reset";
	saip_status st = need_plant(b, fn);
	if (st || (st = need_ready(b, fn))) return st;
	HIP_TRY(hipMemsetAsync(b->plant.summary, 0, (size_t)saip::PLANT_SUMMARY_ROWS * b->ld * sizeof(double), b->stream));
	return SAIP_OK;
}
extern "C" double* saip_batch_plant_joints_device(saip_batch* b) { return b ? b->plant.joints : nullptr; }
extern "C" double* saip_batch_plant_wrenches_device(saip_batch* b) { return b ? b->plant.wrenches : nullptr; }
extern "C" double* saip_batch_plant_torques_device(saip_batch* b) { return b ? b->plant.tau_act : nullptr; }
extern "C" double* saip_batch_plant_summary_device(saip_batch* b) { return b ? b->plant.summary : nullptr; }
// one launch of the plant kernel at the resident state, in front of an integration substep of length dt
static saip_status plant_launch(saip_batch* b, double dt) {
	const auto& C = b->plant;
	saip::PlantParams P;
	memset(&P, 0, sizeof(P));
	P.B = b->B;
	P.ld = b->ld;
	P.n = b->model->n;
	P.n_wrenches = C.n_wrenches;
	P.per_instance_joints = C.per_instance_joints;
	P.per_instance_wrenches = C.per_instance_wrenches;
	P.period = C.period;
	P.dt = dt;
	P.model = b->model_dev;
	P.q = b->q;
	P.dq = b->dq;
	P.tau_cmd = b->tau_bound ? b->tau_bound : b->tau;
	P.joints = C.joints;
	P.wrenches = C.wrenches;
	P.tau_act = C.tau_act;
	P.summary = C.summary;
	for (int k = 0; k < C.n_wrenches; k++) P.site[k] = C.site[k];
	hipError_t e = saip::launch_plant_apply(P, b->model->dev.is_tree != 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "plant launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}

// ---- the step after the path: forward dynamics + semi-implicit Euler on the resident state (saip_dynamics.hip)
static saip_status enqueue_integrate(saip_batch* b, double dt, int substeps, const double* gravity, double damping, bool with_next_otg = false) {
	SimParams S;
	S.B = b->B;
	S.ld = b->ld;
	S.n = b->model->n;
	S.substeps = substeps;
	S.dt = dt;
	S.damping = damping;
	for (int i = 0; i < 3; i++) S.gravity[i] = gravity ? gravity[i] : b->model->dev.gravity[i];
	S.model = b->model_dev;
	S.q = b->q;
	S.dq = b->dq;
	S.tau = b->tau_bound ? b->tau_bound : b->tau;
	S.ddq = nullptr;
	hipError_t e;
	const bool tree = b->model->dev.is_tree != 0;  // trees: the lane-per-instance tree kernel, whatever the dof (the eight-lane step is chain-only)
	if (b->contact.attached || b->n_patch > 0 || b->plant.attached) {
		// contact planes: the penalty force is re-evaluated in front of every substep (held over a control period it is unstable at
		// useful stiffness), and the integrator takes commanded + contact torques; never fused with the next period's OTG step.
		// Contact patches take the same place with their own kernel.  A plant model stands in front of either: it turns the commanded
		// torques into actuated ones, which the contact launch (when there is one) takes in place of the commanded torques; the
		// integrator reads the last buffer written.  The whole call belongs to one period of the plant.
		const bool patches = b->n_patch > 0, contact = patches || b->contact.attached;
		S.substeps = 1;
		S.tau = patches ? b->patch_tau_sim : contact ? b->contact.tau_sim : b->plant.tau_act;
		for (int s = 0; s < substeps; s++) {
			saip_status st = b->plant.attached ? plant_launch(b, dt) : SAIP_OK;
			if (st) return st;
			if (contact) st = patches ? patch_launch(b, saip::CONTACT_APPLY, dt) : contact_launch(b, saip::CONTACT_APPLY, dt);
			if (st) return st;
			e = saip::launch_integrate(S, tree, b->stream);
			if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "integrate launch failed: %s", hipGetErrorString(e));
		}
		if (b->plant.attached) b->plant.period++;
		b->models_valid = false;
		b->state_epoch++;
		return SAIP_OK;
	}
	if (with_next_otg && S.n == 7 && !tree && otg_pair_ready(b)) {
		// rollouts: this integration and the NEXT period's trajectory generation in one launch (they are independent)
		e = saip::launch_integrate_otg_pair(S, b->tasks[0].otg, b->tasks[1].otg, b->B, b->ld, b->stream);
		b->otg_prelaunched = true;
	} else {
		e = saip::launch_integrate(S, tree, b->stream);
	}
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "integrate launch failed: %s", hipGetErrorString(e));
	b->models_valid = false;  // the state moved: like after robot->setQ(), updateControllerTaskModels() is due
	b->state_epoch++;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_integrate(saip_batch* b, double dt, int substeps, const double* gravity, double damping) {
	saip_status st = need_ready(b, "saip_batch_integrate");
	if (st) return st;
	if (!(dt > 0) || substeps < 1 || damping < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_integrate: dt > 0, substeps >= 1, damping >= 0 required");
	return enqueue_integrate(b, dt, substeps, gravity, damping);
}
// ---- rollout recorder (saip_rollout_record.hip): per-period trajectory log and running summaries of saip_batch_rollout_async
static int record_rows(unsigned channels, int n) {
	return ((channels & saip::REC_Q) ? n : 0) + ((channels & saip::REC_DQ) ? n : 0) + ((channels & saip::REC_TAU) ? n : 0) +
		   ((channels & saip::REC_POSE) ? 12 : 0) + ((channels & saip::REC_ERROR) ? 6 : 0);
}
static void record_free(saip_batch* b) {
	auto& R = b->rec;
	for (void* p : {(void*)R.log, (void*)R.status_log, (void*)R.summary})
		if (p) (void)hipFree(p);
	R = saip_batch::Recorder();
}
// the observation of the period that has just been integrated: the sample slot is computed here, at enqueue time (no device-side counter)
static saip_status record_period(saip_batch* b, double T) {
	auto& R = b->rec;
	const long long p = ++R.period;
	const bool sample = R.channels && p % R.stride == 0;
	if (!sample && !R.summary) return SAIP_OK;
	saip::RecordParams P;
	P.B = b->B;
	P.ld = b->ld;
	P.n = b->model->n;
	P.slot = sample ? (int)((p / R.stride - 1) % R.capacity) : -1;
	P.channels = R.channels;
	P.rows = R.rows;
	P.task = R.task;
	P.pad_ = 0;
	P.T = T;
	P.model = b->model_dev;
	P.tasks = b->tasks_dev;
	P.q = b->q;
	P.dq = b->dq;
	P.tau = b->tau_bound ? b->tau_bound : b->tau;
	P.status = b->status;
	P.goal = R.task >= 0 ? b->tasks[R.task].goal_dev : nullptr;
	P.log = R.log;
	P.status_log = R.status_log;
	P.summary = R.summary;
	hipError_t e = saip::launch_rollout_record(P, b->model->dev.is_tree != 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "rollout recorder launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}
// finalized as a controller (no device needed yet: argument errors come first, as in the model queries)
static saip_status need_controller(const saip_batch* b, const char* fn) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null batch", fn);
	if (!b->finalized) return fail(SAIP_ERR_ORDER, "%s: call saip_batch_finalize first", fn);
	if (b->model_only) return fail(SAIP_ERR_ORDER, "%s: the batch was finalized for model queries only (no tasks)", fn);
	return SAIP_OK;
}
static saip_status need_recorder(const saip_batch* b, const char* fn) {
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!b->rec.attached) return fail(SAIP_ERR_ORDER, "%s: no rollout recorder is attached (saip_batch_rollout_recorder_attach)", fn);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_rollout_recorder_attach(saip_batch* b, int capacity, int stride, unsigned channels, int task, int summaries) {
	const char* fn = "saip_batch_rollout_recorder_attach";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (b->rec.attached) return fail(SAIP_ERR_ORDER, "%s: a recorder is already attached (saip_batch_rollout_recorder_detach first)", fn);
	if (capacity < 1 || stride < 1) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: capacity >= 1 and stride >= 1 required", fn);
	if (channels & ~(unsigned)saip::REC_ALL) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: unknown channel bits 0x%x", fn, channels & ~(unsigned)saip::REC_ALL);
	if (!channels && !summaries) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: nothing to record (empty channel mask and no summaries)", fn);
	if (task < -1 || task >= (int)b->tasks.size()) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, task);
	if (task >= 0 && b->tasks[task].dev.type != saip::TASK_MOTION_FORCE) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task %d is not a motion-force task", fn, task);
	if ((channels & (saip::REC_POSE | saip::REC_ERROR)) && task < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the pose and error channels need a motion-force task", fn);
	const int rows = record_rows(channels, b->model->n);
	// [capacity][rows][ld] doubles: the byte count must fit a size_t
	const size_t slot_bytes = (size_t)(rows > 0 ? rows : 1) * b->ld * sizeof(double);
	if ((size_t)capacity > SIZE_MAX / slot_bytes) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: a log of %d samples of %d rows is too large", fn, capacity, rows);
	if ((st = need_ready(b, fn))) return st;
	auto& R = b->rec;
	auto alloc_zero = [&](void** p, size_t bytes) -> saip_status {
		HIP_TRY(hipMalloc(p, bytes));
		HIP_TRY(hipMemset(*p, 0, bytes));
		return SAIP_OK;
	};
	if (channels) {
		if ((st = alloc_zero((void**)&R.log, (size_t)capacity * slot_bytes)) || (st = alloc_zero((void**)&R.status_log, (size_t)capacity * b->ld))) {
			record_free(b);
			return st;
		}
	}
	if (summaries && (st = alloc_zero((void**)&R.summary, (size_t)saip::REC_SUMMARY_ROWS * b->ld * sizeof(double)))) {
		record_free(b);
		return st;
	}
	R.attached = true;
	R.capacity = capacity;
	R.stride = stride;
	R.channels = channels;
	R.task = task;
	R.rows = rows;
	R.period = 0;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_rollout_recorder_detach(saip_batch* b) {
	saip_status st = need_recorder(b, "saip_batch_rollout_recorder_detach");
	if (st) return st;
	if ((st = need_ready(b, "saip_batch_rollout_recorder_detach"))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));  // a recorded period may still be in flight
	record_free(b);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_rollout_recorder_reset(saip_batch* b) {
	saip_status st = need_recorder(b, "saip_batch_rollout_recorder_reset");
	if (st) return st;
	if ((st = need_ready(b, "saip_batch_rollout_recorder_reset"))) return st;
	auto& R = b->rec;
	if (R.log) HIP_TRY(hipMemsetAsync(R.log, 0, (size_t)R.capacity * R.rows * b->ld * sizeof(double), b->stream));
	if (R.status_log) HIP_TRY(hipMemsetAsync(R.status_log, 0, (size_t)R.capacity * b->ld, b->stream));
	if (R.summary) HIP_TRY(hipMemsetAsync(R.summary, 0, (size_t)saip::REC_SUMMARY_ROWS * b->ld * sizeof(double), b->stream));
	R.period = 0;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_rollout_log_info(saip_batch* b, int* n_samples, int* rows, int* first_period, int* stride) {
	saip_status st = need_recorder(b, "saip_batch_rollout_log_info");
	if (st) return st;
	const auto& R = b->rec;
	const long long taken = R.channels ? R.period / R.stride : 0;  // samples written so far; the ring keeps the last `capacity`
	const long long n = taken < R.capacity ? taken : R.capacity;
	if (n_samples) *n_samples = (int)n;
	if (rows) *rows = R.rows;
	if (first_period) *first_period = n ? (int)((taken - n + 1) * R.stride) : 0;
	if (stride) *stride = R.stride;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_rollout_log_host(saip_batch* b, double* out, uint8_t* status) {
	const char* fn = "saip_batch_rollout_log_host";
	saip_status st = need_recorder(b, fn);
	if (st) return st;
	if ((st = need_ready(b, fn))) return st;
	const auto& R = b->rec;
	const long long taken = R.channels ? R.period / R.stride : 0;
	const long long n = taken < R.capacity ? taken : R.capacity;
	// chronological order: the ring from the oldest sample's slot to its end, then from slot 0 (rows of consecutive slots are consecutive
	// [ld] arrays, so each piece is one 2-D copy)
	const long long first = (taken - n) % R.capacity;
	const long long piece[2][2] = {{first, first + n <= R.capacity ? n : R.capacity - first}, {0, first + n <= R.capacity ? 0 : first + n - R.capacity}};
	long long done = 0;
	for (const auto& pc : piece) {
		if (pc[1] == 0) continue;
		if (out)
			HIP_TRY(hipMemcpy2DAsync(out + (size_t)done * R.rows * b->B, (size_t)b->B * sizeof(double), R.log + (size_t)pc[0] * R.rows * b->ld,
									 (size_t)b->ld * sizeof(double), (size_t)b->B * sizeof(double), (size_t)pc[1] * R.rows, hipMemcpyDeviceToHost, b->stream));
		if (status)
			HIP_TRY(hipMemcpy2DAsync(status + (size_t)done * b->B, (size_t)b->B, R.status_log + (size_t)pc[0] * b->ld, (size_t)b->ld, (size_t)b->B,
									 (size_t)pc[1], hipMemcpyDeviceToHost, b->stream));
		done += pc[1];
	}
	HIP_TRY(hipStreamSynchronize(b->stream));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_rollout_summary_host(saip_batch* b, double* out) {
	const char* fn = "saip_batch_rollout_summary_host";
	saip_status st = need_recorder(b, fn);
	if (st) return st;
	if (!b->rec.summary) return fail(SAIP_ERR_ORDER, "%s: the recorder was attached without summaries", fn);
	if (!out) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null output", fn);
	if ((st = need_ready(b, fn))) return st;
	return copy_d2h(b, out, b->rec.summary, saip::REC_SUMMARY_ROWS);
}
extern "C" double* saip_batch_rollout_log_device(saip_batch* b) { return b ? b->rec.log : nullptr; }
extern "C" double* saip_batch_rollout_summary_device(saip_batch* b) { return b ? b->rec.summary : nullptr; }

// ---- goal schedules (saip_goal_schedule.hip): the user goals of every rollout period from keyframes resident on the device
static double sched_max_abs(const double* a, int n) {
	double m = 0;
	for (int i = 0; i < n; i++) m = std::fmax(m, std::fabs(a[i]));
	return m;
}
// LINEAR over the rotation rows: every keyframe orthonormal to 1e-6, consecutive keyframes less than pi - 1e-3 apart.  `at(k, r)`: row r
// (3..11 of the goal block) of keyframe k for the instance under test
template <typename At>
static const char* sched_check_rotations(int K, At at) {
	double prev[9];
	for (int k = 0; k < K; k++) {
		double R[9], G[9];
		for (int e = 0; e < 9; e++) R[e] = at(k, e);
		for (int i = 0; i < 3; i++)
			for (int j = 0; j < 3; j++) G[3 * i + j] = R[i] * R[j] + R[3 + i] * R[3 + j] + R[6 + i] * R[6 + j] - (i == j ? 1.0 : 0.0);
		if (!(sched_max_abs(G, 9) <= 1e-6)) return "a rotation keyframe is not orthonormal (max |R^T R - I| > 1e-6)";
		if (k > 0) {
			double M[9];
			for (int i = 0; i < 3; i++)
				for (int j = 0; j < 3; j++) M[3 * i + j] = prev[i] * R[j] + prev[3 + i] * R[3 + j] + prev[6 + i] * R[6 + j];
			const double w[3] = {0.5 * (M[7] - M[5]), 0.5 * (M[2] - M[6]), 0.5 * (M[3] - M[1])};
			const double angle = std::atan2(std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]), 0.5 * (M[0] + M[4] + M[8] - 1.0));
			if (!(angle <= M_PI - 1e-3)) return "two consecutive rotation keyframes are more than pi - 1e-3 rad apart (the geodesic is ill-defined)";
		}
		for (int e = 0; e < 9; e++) prev[e] = R[e];
	}
	return nullptr;
}
static void sampler_release(saip_batch* b, int task);
static saip_status need_schedule(const saip_batch* b, int task, const char* fn) {
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (task < 0 || task >= (int)b->tasks.size()) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, task);
	if (task >= (int)b->sched.size() || !b->sched[task].attached)
		return fail(SAIP_ERR_ORDER, "%s: task %d has no goal schedule (saip_batch_goal_schedule_attach)", fn, task);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_goal_schedule_attach(saip_batch* b, int task, int first, int count, const double* keyframes, int n_keyframes,
													   int stride, int mode, int per_instance) {
	const char* fn = "saip_batch_goal_schedule_attach";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (task < 0 || task >= (int)b->tasks.size()) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, task);
	if (task < (int)b->sched.size() && b->sched[task].attached)
		return fail(SAIP_ERR_ORDER, "%s: task %d already has a goal schedule (saip_batch_goal_schedule_detach first)", fn, task);
	if (!keyframes) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null keyframes", fn);
	const auto& T = b->tasks[task];
	if (first < 0 || count <= 0 || count > T.dev.goal_comps || first > T.dev.goal_comps - count)
		return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: components [%d, %d + %d) outside the %d goal components of task %d", fn, first, first, count, T.dev.goal_comps, task);
	if (n_keyframes < 1 || stride < 1) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: n_keyframes >= 1 and stride >= 1 required", fn);
	if (b->contact.attached && b->contact.sensor && b->contact.task == task && contact_rows_overlap(first, count))
		return fail(SAIP_ERR_ORDER, "%s: rows 30..35 of task %d are written by the simulated sensor of the attached contact planes", fn, task);
	for (int i = 0; i < b->n_patch; i++)
		if (b->patch[i].sensor && b->patch[i].task == task && contact_rows_overlap(first, count))
			return fail(SAIP_ERR_ORDER, "%s: rows 30..35 of task %d are written by the simulated sensor of its contact patch", fn, task);
	if (mode != saip::SCHED_HOLD && mode != saip::SCHED_LINEAR) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: unknown mode %d", fn, mode);
	per_instance = per_instance ? 1 : 0;
	// [K][count][ld] (or [K][count]) doubles: the byte count must fit a size_t
	const size_t frame_bytes = (size_t)count * (per_instance ? (size_t)b->ld : 1) * sizeof(double);
	if ((size_t)n_keyframes > SIZE_MAX / frame_bytes) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %d keyframes of %d components are too large", fn, n_keyframes, count);
	int rot = 0;
	if (mode == saip::SCHED_LINEAR && T.dev.type == saip::TASK_MOTION_FORCE && first < 12 && first + count > 3) {
		if (first > 3 || first + count < 12)
			return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: a linear schedule must cover all or none of the rotation rows 3..11 (got [%d, %d))", fn, first, first + count);
		rot = 1;
		const size_t B = b->B, r0 = 3 - first;
		const char* bad = nullptr;
		for (size_t i = 0; i < (per_instance ? B : 1) && !bad; i++)
			bad = sched_check_rotations(n_keyframes, [&](int k, int e) {
				const size_t row = (size_t)k * count + r0 + e;
				return per_instance ? keyframes[row * B + i] : keyframes[row];
			});
		if (bad) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: %s", fn, bad);
	}
	if ((st = need_ready(b, fn))) return st;
	double* key = nullptr;
	const size_t bytes = (size_t)n_keyframes * frame_bytes;
	HIP_TRY(hipMalloc((void**)&key, bytes));
	hipError_t e;
	if (per_instance) {
		e = hipMemsetAsync(key, 0, bytes, b->stream);
		if (e == hipSuccess)
			e = hipMemcpy2DAsync(key, (size_t)b->ld * sizeof(double), keyframes, (size_t)b->B * sizeof(double), (size_t)b->B * sizeof(double),
								 (size_t)n_keyframes * count, hipMemcpyHostToDevice, b->stream);
	} else {
		e = hipMemcpyAsync(key, keyframes, bytes, hipMemcpyHostToDevice, b->stream);
	}
	if (e == hipSuccess) e = hipStreamSynchronize(b->stream);  // the host buffer may be reused by the caller right away
	if (e != hipSuccess) {
		(void)hipFree(key);
		return fail(SAIP_ERR_DEVICE, "%s: keyframe upload failed: %s", fn, hipGetErrorString(e));
	}
	if (b->sched.size() < b->tasks.size()) b->sched.resize(b->tasks.size());
	auto& S = b->sched[task];
	S.attached = true;
	S.first = first;
	S.count = count;
	S.K = n_keyframes;
	S.stride = stride;
	S.mode = mode;
	S.per_instance = per_instance;
	S.rot = rot;
	S.key = key;
	b->n_sched++;
	b->sched_period = 0;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_goal_schedule_detach(saip_batch* b, int task) {
	const char* fn = "saip_batch_goal_schedule_detach";
	saip_status st = task == -1 ? need_controller(b, fn) : need_schedule(b, task, fn);
	if (st) return st;
	if (task == -1 && b->n_sched == 0) return SAIP_OK;
	if ((st = need_ready(b, fn))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));  // a scheduled period may still be in flight
	for (int t = 0; t < (int)b->sched.size(); t++) {
		auto& S = b->sched[t];
		if (!S.attached || (task != -1 && t != task)) continue;
		sampler_release(b, t);  // a sampler points into the keyframes: it goes first
		(void)hipFree(S.key);
		S = saip_batch::Schedule();
		b->n_sched--;
	}
	return SAIP_OK;
}
extern "C" saip_status saip_batch_goal_schedule_rewind(saip_batch* b) {
	saip_status st = need_controller(b, "saip_batch_goal_schedule_rewind");
	if (st) return st;
	b->sched_period = 0;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_goal_schedule_info(saip_batch* b, int task, int* first, int* count, int* n_keyframes, int* stride, int* mode,
													 long long* period) {
	saip_status st = need_schedule(b, task, "saip_batch_goal_schedule_info");
	if (st) return st;
	const auto& S = b->sched[task];
	if (first) *first = S.first;
	if (count) *count = S.count;
	if (n_keyframes) *n_keyframes = S.K;
	if (stride) *stride = S.stride;
	if (mode) *mode = S.mode;
	if (period) *period = b->sched_period;
	return SAIP_OK;
}
extern "C" double* saip_batch_goal_schedule_device(saip_batch* b, int task) {
	return (b && task >= 0 && task < (int)b->sched.size()) ? b->sched[task].key : nullptr;
}
// the goals of rollout period c = sched_period, written in front of the period's OTG step and cycle: one launch for every schedule; the
// keyframe index and the fraction are computed here, at enqueue time (no device-side counter)
static saip_status apply_schedules(saip_batch* b) {
	saip::ScheduleParams P;
	memset(&P, 0, sizeof(P));
	P.B = b->B;
	P.ld = b->ld;
	const long long c = b->sched_period++;
	for (int t = 0; t < (int)b->sched.size(); t++) {
		const auto& S = b->sched[t];
		if (!S.attached) continue;
		auto& E = P.e[P.n++];
		E.goal = b->tasks[t].goal_dev;
		E.key = S.key;
		E.first = S.first;
		E.count = S.count;
		E.K = S.K;
		const bool past = c >= (long long)(S.K - 1) * S.stride;  // the last keyframe is held
		E.i = past ? S.K - 1 : (int)(c / S.stride);
		E.s = past ? 0.0 : (double)(c % S.stride) / (double)S.stride;
		E.mode = S.mode;
		E.per_instance = S.per_instance;
		E.rot = S.rot;
	}
	hipError_t e = saip::launch_goal_schedule(P, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "goal schedule launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}

// steps x { internal OTGs, control cycle, integrate } on the engine stream, no host synchronisation.  One period is 3-5 small
// launches.  Plain back-to-back stream launches are the default: they were measured FASTER than replaying a hipGraph of the period
// (68.6 vs 74.2 us per period at B = 4096, 65.7 vs 70.4 us at B = 256, tools/rollout_bench.py) -- the host enqueues far ahead of the
// device either way, and the graph adds inter-node latency.
extern "C" saip_status saip_batch_rollout_async(saip_batch* b, int steps, double sim_dt, int substeps, const double* gravity, double damping) {
	saip_status st = need_ready(b, "saip_batch_rollout_async");
	if (st) return st;
	if (steps < 1 || !(sim_dt > 0) || substeps < 1 || damping < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_rollout_async: bad arguments");
	bool any_otg = false;
	for (auto& T : b->tasks) any_otg = any_otg || T.otg_enabled;
	SimRequest sim = {substeps, sim_dt, damping, {0, 0, 0}};
	for (int i = 0; i < 3; i++) sim.gravity[i] = gravity ? gravity[i] : b->model->dev.gravity[i];
	// with a goal schedule attached every period starts with the launch that writes its goals, and the integration is never fused with
	// the next period's OTG step (which would read the next goal before it is written)
	const bool scheduled = b->n_sched > 0;
	// with contact planes attached neither fused form is used: the contact force sits between the cycle and every integration substep
	// (contact patches: the same, with their kernel)
	// a plant model does the same: it sits between the cycle and every integration substep
	const bool contact = b->contact.attached || b->n_patch > 0 || b->plant.attached;
	const bool patch_sensor = patch_any_sensor(b);
	auto period = [&](const bool more = false) -> saip_status {  // more: another period follows inside this call
		if (scheduled && (st = apply_schedules(b))) return st;
		// contact planes with the simulated sensor: the sensed wrench of this period's state, in front of the OTGs (which pass it on) and the cycle
		if (b->contact.attached && b->contact.sensor && (st = contact_launch(b, saip::CONTACT_SENSE, 0.0))) return st;
		if (patch_sensor && (st = patch_launch(b, saip::CONTACT_SENSE, 0.0))) return st;
		// no internal OTG in the stack: the cycle launch integrates the state itself when it can (eight-lane kernel, no slow path behind)
		bool integrated = false;
		saip_status s2 = launch_cycle(b, false, (!any_otg && b->model->n == 7 && !contact) ? &sim : nullptr, &integrated);
		if (s2) {
			b->otg_prelaunched = false;  // a failed period must not leave the next standalone cycle believing its OTG step has already run
			return s2;
		}
		if (integrated) {  // the bookkeeping of enqueue_integrate
			b->models_valid = false;
			b->state_epoch++;
		} else if ((s2 = enqueue_integrate(b, sim_dt, substeps, gravity, damping, more && !scheduled))) {
			b->otg_prelaunched = false;
			return s2;
		}
		// the clearance monitor observes the integrated state, whichever form integrated it, in front of the recorder
		if (b->clearance.attached && (s2 = clearance_launch(b, saip::CLEARANCE_MONITOR, sim_dt * substeps))) return s2;
		return b->rec.attached ? record_period(b, sim_dt * substeps) : SAIP_OK;
	};
	for (int done = 0; done < steps; done++)
		if ((st = period(done + 1 < steps))) return st;
	return SAIP_OK;
}
// ---- state snapshots (saip_state_snapshot.hip): every per-instance array the engine owns, captured and written back through a
// per-instance source index.  The directory below is the list of those arrays; what is NOT on it is scratch or configuration.
struct SnapSegHost {
	std::string name;
	void* base = nullptr;      // the live array (nullptr on a configuration-only batch)
	int rows = 0, elem_bytes = 0, group = 1, kind = saip::SNAP_SOA;
	size_t bytes = 0;          // of the whole array, padding columns included
	size_t offset = 0;         // of the copy inside the snapshot's arena
};
static void snapshot_directory(const saip_batch* b, std::vector<SnapSegHost>& D) {
	D.clear();
	const size_t ld = b->ld;
	auto soa = [&](const std::string& name, void* base, int rows, int elem) {
		SnapSegHost S;
		S.name = name;
		S.base = base;
		S.rows = rows;
		S.elem_bytes = elem;
		S.bytes = (size_t)rows * ld * elem;
		D.push_back(S);
	};
	const int n = b->model->n;
	soa("q", b->q, n, 8);
	soa("dq", b->dq, n, 8);
	soa("tau", b->tau_bound ? b->tau_bound : b->tau, n, 8);  // whichever the integrator reads
	soa("status", b->status, 1, 1);
	for (size_t t = 0; t < b->tasks.size(); t++) {
		const TaskHost& T = b->tasks[t];
		const std::string p = "task" + std::to_string(t) + ".";
		soa(p + "goal", T.goal_dev, T.dev.goal_comps, 8);
		soa(p + "integ", T.integ_dev, T.integ_rows, 8);
		soa(p + "integ_new", T.integ_new_dev, T.integ_rows, 8);
		if (T.otg_alloc) {
			soa(p + "desired", T.desired_dev, T.dev.goal_comps, 8);
			SnapSegHost S;
			S.name = p + "otg.state";
			S.base = T.otg.state;
			S.rows = saip::otg_state_fields();
			S.elem_bytes = 8;
			S.group = T.otg.gs;
			S.kind = saip::SNAP_GROUPED;
			S.bytes = (size_t)S.rows * (size_t)T.otg.lanes * 8;
			D.push_back(S);
			soa(p + "otg.time", T.otg.time, 1, 8);
			soa(p + "otg.duration", T.otg.duration, 1, 8);
			soa(p + "otg.flags", T.otg.flags, 1, 4);
			soa(p + "otg.seen_epoch", T.otg.seen_epoch, 1, 4);
			soa(p + "otg.result", T.otg.result, 1, 4);
			if (T.otg.frame) soa(p + "otg.frame", T.otg.frame, 21, 8);
		}
		if (T.dev.sh) {
			SnapSegHost S;
			S.name = p + "sh";
			S.base = T.dev.sh;
			S.rows = 1;
			S.elem_bytes = (int)sizeof(saip::ShState);
			S.kind = saip::SNAP_AOS;
			S.bytes = ld * sizeof(saip::ShState);
			D.push_back(S);
		}
		if (T.dev.popc) soa(p + "popc", T.dev.popc, 7 + T.dev.popc_cap, 8);
	}
}
static_assert(sizeof(saip::ShState) % 4 == 0, "ShState is moved as 4- or 8-byte words");
static uint64_t snapshot_fingerprint(const saip_batch* b, const std::vector<SnapSegHost>& D) {
	uint64_t h = 1469598103934665603ull;  // FNV-1a
	auto mix = [&h](const void* p, size_t nb) {
		for (size_t i = 0; i < nb; i++) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
	};
	auto mix_int = [&mix](int v) {
		const int32_t x = v;
		mix(&x, sizeof(x));
	};
	mix_int(b->model->n);
	mix_int(b->B);
	mix_int(b->ld);
	for (const auto& S : D) {
		mix(S.name.c_str(), S.name.size() + 1);
		mix_int(S.rows);
		mix_int(S.elem_bytes);
		mix_int(S.group);
	}
	return h;
}

// the host blob of saip_snapshot_export_host: this header, zero padding up to SNAP_HEADER_BYTES, then the segments at their offsets
struct SnapHeader {
	char magic[8];
	uint32_t version, n_segments;
	uint64_t fingerprint, bytes;
	int32_t otg_prelaunched, n_tasks;
	struct { int32_t sh_cycle, otg_inited; } task[SAIP_MAXT];
};
static const char kSnapMagic[8] = {'S', 'A', 'I', 'P', 'S', 'N', 'A', 'P'};
enum { SNAP_VERSION = 1, SNAP_HEADER_BYTES = 256, SNAP_ALIGN = 256 };
static_assert(sizeof(SnapHeader) == 104 && sizeof(SnapHeader) <= SNAP_HEADER_BYTES, "documented in saip.h");

struct saip_snapshot {
	saip_batch* owner = nullptr;         // nullptr once the batch is gone
	std::vector<SnapSegHost> segs;       // the layout fixed at creation (bases as they were then)
	uint64_t fingerprint = 0;
	size_t arena_bytes = 0;
	char* arena = nullptr;               // the copies, at segs[i].offset
	saip::SnapSeg* table = nullptr;      // [segs] device
	int* unit_seg = nullptr;             // [units] device: segment of every work unit
	int units = 0;
	int* map_dev = nullptr;              // [B]
	int* map_stage = nullptr;            // [B] pinned: the host map on its way to map_dev
	hipEvent_t map_ev = nullptr;         // the last upload from map_stage
	bool map_busy = false;
	bool filled = false;                 // a save or an import has happened: there is something to restore
	SnapHeader host;                     // the host scalars of the last save / import (and the header of an export)
};
static void snapshot_release_device(saip_snapshot* s) {
	if (s->map_ev) (void)hipEventDestroy(s->map_ev);
	for (void* p : {(void*)s->arena, (void*)s->table, (void*)s->unit_seg, (void*)s->map_dev})
		if (p) (void)hipFree(p);
	if (s->map_stage) (void)hipHostFree(s->map_stage);
	s->arena = nullptr;
	s->table = nullptr;
	s->unit_seg = nullptr;
	s->map_dev = s->map_stage = nullptr;
	s->map_ev = nullptr;
	s->owner = nullptr;
}
static size_t snapshot_layout(std::vector<SnapSegHost>& D) {  // arena offsets; returns the arena size
	size_t at = 0;
	for (auto& S : D) {
		S.offset = at;
		at += (S.bytes + SNAP_ALIGN - 1) / SNAP_ALIGN * SNAP_ALIGN;
	}
	return at;
}
static void snapshot_host_scalars(const saip_batch* b, SnapHeader& H) {
	H.otg_prelaunched = b->otg_prelaunched ? 1 : 0;
	H.n_tasks = (int32_t)b->tasks.size();
	for (int t = 0; t < SAIP_MAXT; t++) {
		H.task[t].sh_cycle = t < (int)b->tasks.size() ? b->tasks[t].sh_cycle : 0;
		H.task[t].otg_inited = t < (int)b->tasks.size() && b->tasks[t].otg_inited ? 1 : 0;
	}
}
// the batch's directory as it is now against the snapshot's: the first segment that differs is named
static saip_status snapshot_match(saip_batch* b, const saip_snapshot* s, const char* fn) {
	if (s->owner != b) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the snapshot belongs to another batch (a snapshot restores only into the batch that created it)", fn);
	if (!s->filled && strcmp(fn, "saip_batch_snapshot_save") != 0)
		return fail(SAIP_ERR_ORDER, "%s: the snapshot is empty (saip_batch_snapshot_save or saip_snapshot_import_host first)", fn);
	saip_status st = ensure_lazy_state(b);
	if (st) return st;
	std::vector<SnapSegHost> D;
	snapshot_directory(b, D);
	const size_t n = D.size() < s->segs.size() ? D.size() : s->segs.size();
	for (size_t i = 0; i <= n; i++) {
		const SnapSegHost* a = i < D.size() ? &D[i] : nullptr;
		const SnapSegHost* c = i < s->segs.size() ? &s->segs[i] : nullptr;
		if (!a && !c) break;
		if (!a || !c)
			return fail(SAIP_ERR_ORDER, "%s: the state layout changed since the snapshot was created: segment [%s] %s (create a new snapshot)", fn,
						(a ? a : c)->name.c_str(), a ? "is new" : "is gone");
		if (a->name != c->name || a->rows != c->rows || a->elem_bytes != c->elem_bytes || a->group != c->group || a->kind != c->kind)
			return fail(SAIP_ERR_ORDER, "%s: the state layout changed since the snapshot was created: segment [%s] where the snapshot has [%s] (create a new snapshot)",
						fn, a->name.c_str(), c->name.c_str());
		if (a->base != c->base)
			return fail(SAIP_ERR_ORDER, "%s: segment [%s] lives in another array than when the snapshot was created (create a new snapshot)", fn, a->name.c_str());
	}
	return SAIP_OK;
}
extern "C" saip_status saip_batch_snapshot_create(saip_batch* b, saip_snapshot** out) {
	const char* fn = "saip_batch_snapshot_create";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!out) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null output", fn);
	if ((st = need_ready(b, fn))) return st;
	if ((st = ensure_lazy_state(b))) return st;
	auto* s = new saip_snapshot();
	s->owner = b;
	snapshot_directory(b, s->segs);
	s->fingerprint = snapshot_fingerprint(b, s->segs);
	s->arena_bytes = snapshot_layout(s->segs);
	// the device table: one SnapSeg per segment, and the segment of every work unit
	std::vector<saip::SnapSeg> table;
	std::vector<int> unit_seg;
	long long units = 0;
	for (const auto& H : s->segs) {
		saip::SnapSeg S;
		memset(&S, 0, sizeof(S));
		S.rows = H.rows;
		if (H.kind == saip::SNAP_SOA) {
			S.wpi = 1;
			S.word_bytes = H.elem_bytes;
			S.row_stride = b->ld;
		} else if (H.kind == saip::SNAP_GROUPED) {
			S.wpi = H.group;
			S.word_bytes = 8;
			S.row_stride = (long long)b->B * H.group;
		} else {
			S.word_bytes = H.elem_bytes % 8 == 0 ? 8 : 4;
			S.wpi = H.elem_bytes / S.word_bytes;
			S.row_stride = 0;
		}
		S.words = (long long)b->B * S.wpi;
		const long long chunks = (S.words + saip::SNAP_CHUNK - 1) / saip::SNAP_CHUNK;
		const long long u = chunks * ((S.rows + saip::SNAP_ROWS - 1) / saip::SNAP_ROWS);
		if (units + u > 0x7fffffffll) {
			delete s;
			return fail(SAIP_ERR_UNSUPPORTED, "%s: the state of this batch is too large for one gather launch", fn);
		}
		S.chunks = (int)chunks;
		S.unit0 = (int)units;
		units += u;
		unit_seg.insert(unit_seg.end(), (size_t)u, (int)table.size());
		table.push_back(S);
	}
	s->units = (int)units;
	auto cleanup = [&](saip_status e) {
		snapshot_release_device(s);
		delete s;
		return e;
	};
	auto alloc = [&](void** p, size_t bytes) -> saip_status {
		HIP_TRY(hipMalloc(p, bytes ? bytes : 1));
		return SAIP_OK;
	};
	if ((st = alloc((void**)&s->arena, s->arena_bytes)) || (st = alloc((void**)&s->table, table.size() * sizeof(saip::SnapSeg))) ||
		(st = alloc((void**)&s->unit_seg, unit_seg.size() * sizeof(int))) || (st = alloc((void**)&s->map_dev, (size_t)b->B * sizeof(int))))
		return cleanup(st);
	if (hipHostMalloc((void**)&s->map_stage, (size_t)b->B * sizeof(int), hipHostMallocDefault) != hipSuccess || hipEventCreateWithFlags(&s->map_ev, hipEventDisableTiming) != hipSuccess)
		return cleanup(fail(SAIP_ERR_DEVICE, "%s: could not allocate the map staging buffer", fn));
	for (size_t i = 0; i < table.size(); i++) {
		table[i].live = (char*)s->segs[i].base;
		table[i].snap = s->arena + s->segs[i].offset;
	}
	if (hipMemsetAsync(s->arena, 0, s->arena_bytes ? s->arena_bytes : 1, b->stream) != hipSuccess ||
		hipMemcpyAsync(s->table, table.data(), table.size() * sizeof(saip::SnapSeg), hipMemcpyHostToDevice, b->stream) != hipSuccess ||
		hipMemcpyAsync(s->unit_seg, unit_seg.data(), unit_seg.size() * sizeof(int), hipMemcpyHostToDevice, b->stream) != hipSuccess ||
		hipStreamSynchronize(b->stream) != hipSuccess)  // table and unit_seg are stack objects
		return cleanup(fail(SAIP_ERR_DEVICE, "%s: could not write the segment table", fn));
	memset(&s->host, 0, sizeof(s->host));
	memcpy(s->host.magic, kSnapMagic, 8);
	s->host.version = SNAP_VERSION;
	s->host.n_segments = (uint32_t)s->segs.size();
	s->host.fingerprint = s->fingerprint;
	s->host.bytes = SNAP_HEADER_BYTES + s->arena_bytes;
	snapshot_host_scalars(b, s->host);
	b->snapshots.push_back(s);
	*out = s;
	return SAIP_OK;
}
extern "C" void saip_snapshot_destroy(saip_snapshot* s) {
	if (!s) return;
	if (s->owner) {
		saip_batch* b = s->owner;
		(void)hipSetDevice(b->device);
		if (b->stream) (void)hipStreamSynchronize(b->stream);  // a save or restore may still be in flight
		for (size_t i = 0; i < b->snapshots.size(); i++)
			if (b->snapshots[i] == s) {
				b->snapshots.erase(b->snapshots.begin() + i);
				break;
			}
		snapshot_release_device(s);
	}
	delete s;
}
// entry checks shared by save / restore / export: arguments first, then the device, then the layout
static saip_status snapshot_ready(saip_batch* b, const saip_snapshot* s, const char* fn) {
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!s) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null snapshot", fn);
	if ((st = need_ready(b, fn))) return st;
	return snapshot_match(b, s, fn);
}
extern "C" saip_status saip_batch_snapshot_save(saip_batch* b, saip_snapshot* s) {
	const char* fn = "saip_batch_snapshot_save";
	saip_status st = snapshot_ready(b, s, fn);
	if (st) return st;
	hipError_t e = saip::launch_state_gather(s->table, s->unit_seg, s->units, b->B, nullptr, 1, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "%s: launch failed: %s", fn, hipGetErrorString(e));
	snapshot_host_scalars(b, s->host);
	s->filled = true;
	return SAIP_OK;
}
static saip_status snapshot_restore(saip_batch* b, const saip_snapshot* s, const int* map_dev, const char* fn) {
	hipError_t e = saip::launch_state_gather(s->table, s->unit_seg, s->units, b->B, map_dev, 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "%s: launch failed: %s", fn, hipGetErrorString(e));
	// the host scalars that give the restored arrays their meaning; the restored state is a new state
	for (size_t t = 0; t < b->tasks.size(); t++) {
		b->tasks[t].sh_cycle = s->host.task[t].sh_cycle;
		b->tasks[t].otg_inited = s->host.task[t].otg_inited != 0;
	}
	b->otg_prelaunched = s->host.otg_prelaunched != 0;
	b->models_valid = false;
	b->state_epoch++;
	b->state_pushed = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_snapshot_restore(saip_batch* b, const saip_snapshot* cs, const int* src_host) {
	const char* fn = "saip_batch_snapshot_restore";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!cs) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null snapshot", fn);
	if (src_host)
		for (int i = 0; i < b->B; i++)
			if (src_host[i] < 0 || src_host[i] >= b->B)
				return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: source index %d of instance %d is outside 0 .. %d", fn, src_host[i], i, b->B - 1);
	if ((st = need_ready(b, fn))) return st;
	if ((st = snapshot_match(b, cs, fn))) return st;
	if (!src_host) return snapshot_restore(b, cs, nullptr, fn);
	saip_snapshot* s = const_cast<saip_snapshot*>(cs);  // the staging buffer is the snapshot's own scratch, not part of what it holds
	if (s->map_busy) HIP_TRY(hipEventSynchronize(s->map_ev));  // the previous map has left the staging buffer (that upload only, not the device)
	memcpy(s->map_stage, src_host, (size_t)b->B * sizeof(int));
	HIP_TRY(hipMemcpyAsync(s->map_dev, s->map_stage, (size_t)b->B * sizeof(int), hipMemcpyHostToDevice, b->stream));
	HIP_TRY(hipEventRecord(s->map_ev, b->stream));
	s->map_busy = true;
	return snapshot_restore(b, s, s->map_dev, fn);
}
extern "C" saip_status saip_batch_snapshot_restore_device(saip_batch* b, const saip_snapshot* s, const int* src_dev) {
	const char* fn = "saip_batch_snapshot_restore_device";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!s) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null snapshot", fn);
	if (!src_dev) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null source map", fn);
	if ((st = need_ready(b, fn))) return st;
	if ((st = snapshot_match(b, s, fn))) return st;
	return snapshot_restore(b, s, src_dev, fn);
}
extern "C" int saip_snapshot_segments(const saip_snapshot* s) { return s ? (int)s->segs.size() : 0; }
extern "C" saip_status saip_snapshot_segment_info(const saip_snapshot* s, int i, const char** name, int* rows, int* elem_bytes, int* group, int* kind, size_t* offset) {
	if (!s) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_snapshot_segment_info: null snapshot");
	if (i < 0 || i >= (int)s->segs.size()) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_snapshot_segment_info: segment %d out of range (%d segments)", i, (int)s->segs.size());
	const SnapSegHost& S = s->segs[i];
	if (name) *name = S.name.c_str();
	if (rows) *rows = S.rows;
	if (elem_bytes) *elem_bytes = S.elem_bytes;
	if (group) *group = S.group;
	if (kind) *kind = S.kind;
	if (offset) *offset = SNAP_HEADER_BYTES + S.offset;
	return SAIP_OK;
}
extern "C" size_t saip_snapshot_bytes(const saip_snapshot* s) { return s ? SNAP_HEADER_BYTES + s->arena_bytes : 0; }
extern "C" saip_status saip_snapshot_export_host(saip_batch* b, const saip_snapshot* s, void* out, size_t bytes) {
	const char* fn = "saip_snapshot_export_host";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!s || !out) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null argument", fn);
	if (s->owner != b) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the snapshot belongs to another batch", fn);
	if (bytes < SNAP_HEADER_BYTES + s->arena_bytes)
		return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the buffer holds %zu bytes, the snapshot needs %zu (saip_snapshot_bytes)", fn, bytes, SNAP_HEADER_BYTES + s->arena_bytes);
	if ((st = need_ready(b, fn))) return st;
	memset(out, 0, SNAP_HEADER_BYTES);
	memcpy(out, &s->host, sizeof(SnapHeader));
	if (s->arena_bytes) HIP_TRY(hipMemcpyAsync((char*)out + SNAP_HEADER_BYTES, s->arena, s->arena_bytes, hipMemcpyDeviceToHost, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));
	return SAIP_OK;
}
extern "C" saip_status saip_snapshot_import_host(saip_batch* b, saip_snapshot* s, const void* in, size_t bytes) {
	const char* fn = "saip_snapshot_import_host";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (!in) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null buffer", fn);
	// the blob against the layout of this batch: nothing here needs the device
	if (bytes < SNAP_HEADER_BYTES) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: short buffer: %zu bytes do not hold the %d-byte header", fn, bytes, (int)SNAP_HEADER_BYTES);
	SnapHeader H;
	memcpy(&H, in, sizeof(H));
	if (memcmp(H.magic, kSnapMagic, 8) != 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: bad magic: not a state snapshot", fn);
	if (H.version != SNAP_VERSION) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: snapshot format version %u, this library reads version %d", fn, H.version, (int)SNAP_VERSION);
	std::vector<SnapSegHost> D;
	if (s) D = s->segs;
	else snapshot_directory(b, D);
	const uint64_t fp = s ? s->fingerprint : snapshot_fingerprint(b, D);
	const size_t need = SNAP_HEADER_BYTES + (s ? s->arena_bytes : snapshot_layout(D));
	if (H.fingerprint != fp)
		return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: wrong fingerprint: the blob was taken from another state layout (%016llx, expected %016llx)", fn,
					(unsigned long long)H.fingerprint, (unsigned long long)fp);
	if (H.n_segments != D.size() || H.n_tasks != (int32_t)b->tasks.size() || H.bytes != need)
		return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: inconsistent header (%u segments, %d tasks, %llu bytes)", fn, H.n_segments, (int)H.n_tasks, (unsigned long long)H.bytes);
	if (bytes < need) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: short buffer: %zu bytes, the snapshot has %zu", fn, bytes, need);
	if (!s) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null snapshot", fn);
	if (s->owner != b) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the snapshot belongs to another batch", fn);
	if ((st = need_ready(b, fn))) return st;
	if (s->arena_bytes) HIP_TRY(hipMemcpyAsync(s->arena, (const char*)in + SNAP_HEADER_BYTES, s->arena_bytes, hipMemcpyHostToDevice, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));  // the caller's buffer may be reused right away
	s->host = H;
	s->filled = true;
	return SAIP_OK;
}

// ---- resident rollout sampler (saip_sampler.hip): perturb the resident keyframes around a nominal plan, one cost per instance from
// the recorder, softmin update of the plan -- the steps of a sampling-MPC round that would otherwise go through the host
static_assert(saip::SAMP_MAXT == SAIP_MAXT && saip::SAMP_SUMMARY_ROWS == saip::REC_SUMMARY_ROWS, "saip_sampler.h restates them");
static void sampler_release(saip_batch* b, int task) {  // the stream is idle
	if (task >= (int)b->samp.size() || !b->samp[task].attached) return;
	(void)hipFree(b->samp[task].nominal);
	b->samp[task] = saip_batch::Sampler();
	if (--b->n_samp > 0) return;
	for (void* p : {(void*)b->samp_cost, (void*)b->samp_w, (void*)b->samp_best_map, (void*)b->samp_result})
		if (p) (void)hipFree(p);
	b->samp_cost = b->samp_w = nullptr;
	b->samp_best_map = nullptr;
	b->samp_result = nullptr;
}
// any sampler entry: a controller with at least one sampler (task >= 0: that task's)
static saip_status need_sampler(const saip_batch* b, int task, const char* fn) {
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (task >= (int)b->tasks.size()) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, task);
	if (b->n_samp == 0 || (task >= 0 && (task >= (int)b->samp.size() || !b->samp[task].attached)))
		return fail(SAIP_ERR_ORDER, "%s: no sampler is attached%s (saip_batch_sampler_attach)", fn, task >= 0 ? " to this task" : "");
	return SAIP_OK;
}
static void sampler_params(const saip_batch* b, saip::SamplerParams& P) {
	memset(&P, 0, sizeof(P));
	P.B = b->B;
	P.ld = b->ld;
	P.seed_lo = (uint32_t)b->samp_seed;
	P.seed_hi = (uint32_t)(b->samp_seed >> 32);
	P.round = (uint32_t)b->samp_round;
	for (int t = 0; t < (int)b->samp.size(); t++) {
		const auto& S = b->samp[t];
		if (!S.attached) continue;
		const auto& H = b->sched[t];
		auto& E = P.e[P.n++];
		E.key = H.key;
		E.nominal = S.nominal;
		E.sigma = S.nominal + (size_t)H.K * H.count;
		E.count = H.count;
		E.K = H.K;
		E.d = S.d;
		E.rot = S.rot;
		E.r_rot = S.r_rot;
		E.task = t;
		E.exempt = S.exempt;
	}
}
extern "C" saip_status saip_batch_sampler_attach(saip_batch* b, int task, const double* sigma, const double* nominal, int exempt) {
	const char* fn = "saip_batch_sampler_attach";
	saip_status st = need_controller(b, fn);
	if (st) return st;
	if (task < 0 || task >= (int)b->tasks.size()) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, task);
	if (!sigma) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null sigma", fn);
	if (exempt < 0 || exempt > b->B) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: exempt = %d outside 0 .. %d", fn, exempt, b->B);
	if (task >= (int)b->sched.size() || !b->sched[task].attached)
		return fail(SAIP_ERR_ORDER, "%s: task %d has no goal schedule (saip_batch_goal_schedule_attach first)", fn, task);
	if (task < (int)b->samp.size() && b->samp[task].attached)
		return fail(SAIP_ERR_ORDER, "%s: task %d already has a sampler (saip_batch_sampler_detach first)", fn, task);
	const auto& H = b->sched[task];
	if (!H.per_instance) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the schedule of task %d is batch-uniform; a sampler needs per-instance keyframes", fn, task);
	int rot = 0, r_rot = H.count;
	if (b->tasks[task].dev.type == saip::TASK_MOTION_FORCE && H.first < 12 && H.first + H.count > 3) {
		if (H.first > 3 || H.first + H.count < 12)
			return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: a sampled schedule must cover all or none of the rotation rows 3..11 (got [%d, %d))", fn, H.first, H.first + H.count);
		rot = 1;
		r_rot = 3 - H.first;
	}
	if (H.count > saip::SAMP_MAX_ROWS)
		return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: the schedule of task %d covers %d rows; a sampler takes at most %d", fn, task, H.count, (int)saip::SAMP_MAX_ROWS);
	const int d = rot ? H.count - 6 : H.count;
	for (int j = 0; j < d; j++)
		if (!(sigma[j] >= 0) || !std::isfinite(sigma[j])) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: sigma[%d] = %g is negative or not finite", fn, j, sigma[j]);
	if (nominal && rot && H.mode == saip::SCHED_LINEAR) {
		const int count = H.count;
		const char* bad = sched_check_rotations(H.K, [&](int k, int e) { return nominal[(size_t)k * count + r_rot + e]; });
		if (bad) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: nominal plan: %s", fn, bad);
	}
	if ((st = need_ready(b, fn))) return st;
	const size_t plan = (size_t)H.K * H.count;
	double* dev = nullptr;
	HIP_TRY(hipMalloc((void**)&dev, (plan + d) * sizeof(double)));
	const bool first = b->n_samp == 0;
	hipError_t e = hipSuccess;
	if (first) {
		const size_t ld = b->ld;
		if ((e = hipMalloc((void**)&b->samp_cost, ld * sizeof(double))) == hipSuccess && (e = hipMalloc((void**)&b->samp_w, ld * sizeof(double))) == hipSuccess &&
			(e = hipMalloc((void**)&b->samp_best_map, ld * sizeof(int))) == hipSuccess && (e = hipMalloc((void**)&b->samp_result, sizeof(saip::SamplerResult))) == hipSuccess &&
			(e = hipMemsetAsync(b->samp_cost, 0, ld * sizeof(double), b->stream)) == hipSuccess && (e = hipMemsetAsync(b->samp_w, 0, ld * sizeof(double), b->stream)) == hipSuccess &&
			(e = hipMemsetAsync(b->samp_best_map, 0xff, ld * sizeof(int), b->stream)) == hipSuccess) {  // the map starts at -1: no best yet
			saip::SamplerResult none = {-1, 0, 0.0, 0.0, 0.0};
			e = hipMemcpyAsync(b->samp_result, &none, sizeof(none), hipMemcpyHostToDevice, b->stream);
			if (e == hipSuccess) e = hipStreamSynchronize(b->stream);  // `none` is a stack object
		}
	}
	if (e == hipSuccess) {
		if (nominal) e = hipMemcpyAsync(dev, nominal, plan * sizeof(double), hipMemcpyHostToDevice, b->stream);
		else {  // column 0 of the resident keyframes, through the host (an attach waits for the stream anyway)
			std::vector<double> col(plan);
			e = hipMemcpy2DAsync(col.data(), sizeof(double), H.key, (size_t)b->ld * sizeof(double), sizeof(double), plan, hipMemcpyDeviceToHost, b->stream);
			if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
			if (e == hipSuccess) e = hipMemcpy(dev, col.data(), plan * sizeof(double), hipMemcpyHostToDevice);
		}
	}
	if (e == hipSuccess) e = hipMemcpyAsync(dev + plan, sigma, (size_t)d * sizeof(double), hipMemcpyHostToDevice, b->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(b->stream);  // the host buffers may be reused by the caller right away
	if (e != hipSuccess) {
		(void)hipFree(dev);
		if (first) {
			for (void* p : {(void*)b->samp_cost, (void*)b->samp_w, (void*)b->samp_best_map, (void*)b->samp_result})
				if (p) (void)hipFree(p);
			b->samp_cost = b->samp_w = nullptr;
			b->samp_best_map = nullptr;
			b->samp_result = nullptr;
		}
		return fail(SAIP_ERR_DEVICE, "%s: upload failed: %s", fn, hipGetErrorString(e));
	}
	if (b->samp.size() < b->tasks.size()) b->samp.resize(b->tasks.size());
	auto& S = b->samp[task];
	S.attached = true;
	S.d = d;
	S.rot = rot;
	S.r_rot = r_rot;
	S.exempt = exempt;
	S.nominal = dev;
	b->n_samp++;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sampler_detach(saip_batch* b, int task) {
	const char* fn = "saip_batch_sampler_detach";
	if (task < -1) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, task);
	saip_status st = need_sampler(b, task, fn);
	if (st) return st;
	if ((st = need_ready(b, fn))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));  // a sampler launch may still be in flight
	for (int t = (int)b->samp.size() - 1; t >= 0; t--)
		if (task == -1 || t == task) sampler_release(b, t);
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sampler_seed(saip_batch* b, unsigned long long seed) {
	saip_status st = need_sampler(b, -1, "saip_batch_sampler_seed");
	if (st) return st;
	b->samp_seed = seed;
	b->samp_round = 0;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sampler_perturb(saip_batch* b) {
	const char* fn = "saip_batch_sampler_perturb";
	saip_status st = need_sampler(b, -1, fn);
	if (st) return st;
	if ((st = need_ready(b, fn))) return st;
	saip::SamplerParams P;
	sampler_params(b, P);
	hipError_t e = saip::launch_sampler_perturb(P, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "%s: launch failed: %s", fn, hipGetErrorString(e));
	b->samp_round++;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sampler_cost(saip_batch* b, const double* w_summary, const double* target, double w_path, double w_final) {
	const char* fn = "saip_batch_sampler_cost";
	saip_status st = need_sampler(b, -1, fn);
	if (st) return st;
	const auto& R = b->rec;
	saip::SamplerCostParams P;
	memset(&P, 0, sizeof(P));
	bool any_w = false;
	for (int r = 0; w_summary && r < saip::REC_SUMMARY_ROWS; r++) {
		P.w[r] = w_summary[r];
		any_w = any_w || w_summary[r] != 0.0;
	}
	if (any_w && !(R.attached && R.summary)) return fail(SAIP_ERR_ORDER, "%s: a summary weight is set but no recorder keeps summaries (saip_batch_rollout_recorder_attach)", fn);
	if (target) {
		if (!R.attached || !(R.channels & saip::REC_POSE)) return fail(SAIP_ERR_ORDER, "%s: a target needs the recorder's POSE channel", fn);
		const long long taken = R.period / R.stride;
		if (taken < 1) return fail(SAIP_ERR_ORDER, "%s: a target needs at least one recorded sample", fn);
		const long long n = taken < R.capacity ? taken : R.capacity;
		const int dof = b->model->n;
		P.log = R.log;
		P.rows = R.rows;
		P.pose_row0 = ((R.channels & saip::REC_Q) ? dof : 0) + ((R.channels & saip::REC_DQ) ? dof : 0) + ((R.channels & saip::REC_TAU) ? dof : 0);
		P.capacity = R.capacity;
		P.first_slot = (int)((taken - n) % R.capacity);  // the ring in chronological order, as saip_batch_rollout_log_host reads it
		P.n_samples = (int)n;
		P.has_target = 1;
		for (int i = 0; i < 3; i++) P.target[i] = target[i];
		P.w_path = w_path;
		P.w_final = w_final;
	}
	if ((st = need_ready(b, fn))) return st;
	P.B = b->B;
	P.ld = b->ld;
	P.summary = any_w ? R.summary : nullptr;
	P.cost = b->samp_cost;
	hipError_t e = saip::launch_sampler_cost(P, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "%s: launch failed: %s", fn, hipGetErrorString(e));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sampler_set_cost_host(saip_batch* b, const double* cost) {
	const char* fn = "saip_batch_sampler_set_cost_host";
	saip_status st = need_sampler(b, -1, fn);
	if (st) return st;
	if (!cost) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null cost", fn);
	if ((st = need_ready(b, fn))) return st;
	return copy_h2d(b, b->samp_cost, cost, 1);
}
extern "C" saip_status saip_batch_sampler_get_cost_host(saip_batch* b, double* cost) {
	const char* fn = "saip_batch_sampler_get_cost_host";
	saip_status st = need_sampler(b, -1, fn);
	if (st) return st;
	if (!cost) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null output", fn);
	if ((st = need_ready(b, fn))) return st;
	return copy_d2h(b, cost, b->samp_cost, 1);
}
extern "C" double* saip_batch_sampler_cost_device(saip_batch* b) { return b ? b->samp_cost : nullptr; }
extern "C" const int* saip_batch_sampler_best_map_device(saip_batch* b) { return b ? b->samp_best_map : nullptr; }
extern "C" saip_status saip_batch_sampler_update(saip_batch* b, double temperature) {
	const char* fn = "saip_batch_sampler_update";
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null batch", fn);
	if (!(temperature > 0) || !std::isfinite(temperature)) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: temperature = %g: a finite value > 0 is required", fn, temperature);
	saip_status st = need_sampler(b, -1, fn);
	if (st) return st;
	if ((st = need_ready(b, fn))) return st;
	saip::SamplerParams P;
	sampler_params(b, P);
	hipError_t e = saip::launch_sampler_update(P, b->samp_cost, temperature, b->samp_w, b->samp_result, b->samp_best_map, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "%s: launch failed: %s", fn, hipGetErrorString(e));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sampler_shift(saip_batch* b, int n) {
	const char* fn = "saip_batch_sampler_shift";
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null batch", fn);
	if (n < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: n = %d is negative", fn, n);
	saip_status st = need_sampler(b, -1, fn);
	if (st) return st;
	if ((st = need_ready(b, fn))) return st;
	if (n == 0) return SAIP_OK;
	saip::SamplerParams P;
	sampler_params(b, P);
	hipError_t e = saip::launch_sampler_shift(P, n, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "%s: launch failed: %s", fn, hipGetErrorString(e));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sampler_result_host(saip_batch* b, int* best, int* n_valid, double* min_cost, double* sum_w, double* ess) {
	const char* fn = "saip_batch_sampler_result_host";
	saip_status st = need_sampler(b, -1, fn);
	if (st) return st;
	if ((st = need_ready(b, fn))) return st;
	saip::SamplerResult r;
	HIP_TRY(hipMemcpyAsync(&r, b->samp_result, sizeof(r), hipMemcpyDeviceToHost, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));
	if (best) *best = r.best;
	if (n_valid) *n_valid = r.n_valid;
	if (min_cost) *min_cost = r.min_cost;
	if (sum_w) *sum_w = r.sum_w;
	if (ess) *ess = r.ess;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sampler_get_nominal_host(saip_batch* b, int task, double* out) {
	const char* fn = "saip_batch_sampler_get_nominal_host";
	if (task < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, task);
	saip_status st = need_sampler(b, task, fn);
	if (st) return st;
	if (!out) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null output", fn);
	if ((st = need_ready(b, fn))) return st;
	HIP_TRY(hipMemcpyAsync(out, b->samp[task].nominal, (size_t)b->sched[task].K * b->sched[task].count * sizeof(double), hipMemcpyDeviceToHost, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sampler_set_nominal_host(saip_batch* b, int task, const double* in) {
	const char* fn = "saip_batch_sampler_set_nominal_host";
	if (task < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, task);
	saip_status st = need_sampler(b, task, fn);
	if (st) return st;
	if (!in) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null nominal plan", fn);
	if (b->samp[task].rot && b->sched[task].mode == saip::SCHED_LINEAR) {  // as _attach checks it
		const int count = b->sched[task].count, r_rot = b->samp[task].r_rot;
		const char* bad = sched_check_rotations(b->sched[task].K, [&](int k, int e) { return in[(size_t)k * count + r_rot + e]; });
		if (bad) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: nominal plan: %s", fn, bad);
	}
	if ((st = need_ready(b, fn))) return st;
	HIP_TRY(hipMemcpyAsync(b->samp[task].nominal, in, (size_t)b->sched[task].K * b->sched[task].count * sizeof(double), hipMemcpyHostToDevice, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));  // the host buffer may be reused by the caller right away
	return SAIP_OK;
}
extern "C" saip_status saip_batch_sampler_info(saip_batch* b, int task, int* d, int* exempt, unsigned long long* seed, long long* round) {
	const char* fn = "saip_batch_sampler_info";
	if (task < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: task id %d out of range", fn, task);
	saip_status st = need_sampler(b, task, fn);
	if (st) return st;
	if (d) *d = b->samp[task].d;
	if (exempt) *exempt = b->samp[task].exempt;
	if (seed) *seed = b->samp_seed;
	if (round) *round = b->samp_round;
	return SAIP_OK;
}

extern "C" saip_status saip_batch_set_torques_host(saip_batch* b, const double* tau) {
	saip_status st = need_ready(b, "saip_batch_set_torques_host");
	if (st) return st;
	if (!tau) return fail(SAIP_ERR_INVALID_ARGUMENT, "null torque pointer");
	return copy_h2d(b, b->tau_bound ? b->tau_bound : b->tau, tau, b->model->n);
}
extern "C" saip_status saip_batch_get_state_host(saip_batch* b, double* q, double* dq) {
	saip_status st = need_state(b, "saip_batch_get_state_host");
	if (st) return st;
	if (q && (st = copy_d2h(b, q, b->q, b->model->n))) return st;
	if (dq && (st = copy_d2h(b, dq, b->dq, b->model->n))) return st;
	return SAIP_OK;
}

// desired state of a task = what its control law tracks: the internal OTG's output when enabled, else the goal (JointTask.h:185-200)
extern "C" saip_status saip_batch_get_desired_host(saip_batch* b, int t, double* desired) {
	saip_status st = need_ready(b, "saip_batch_get_desired_host");
	if (st) return st;
	if ((st = check_batch(b, t, "saip_batch_get_desired_host"))) return st;
	if (t < 0 || !desired) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_get_desired_host: bad argument");
	TaskHost& T = b->tasks[t];
	const bool otg = T.otg_enabled && T.otg_alloc && T.otg_inited;
	return copy_d2h(b, desired, otg ? T.desired_dev : T.goal_dev, T.dev.goal_comps);
}
extern "C" saip_status saip_batch_get_otg_status_host(saip_batch* b, int t, int* flags, int* result) {
	saip_status st = check_batch(b, t, "saip_batch_get_otg_status_host");
	if (st) return st;
	if (t < 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad task");
	if ((st = need_ready(b, "saip_batch_get_otg_status_host"))) return st;
	TaskHost& T = b->tasks[t];
	if (!T.otg_alloc) return fail(SAIP_ERR_ORDER, "saip_batch_get_otg_status_host: the internal OTG of task [%s] has not run", T.name.c_str());
	if (flags) HIP_TRY(hipMemcpyAsync(flags, T.otg.flags, (size_t)b->B * sizeof(int), hipMemcpyDeviceToHost, b->stream));
	if (result) HIP_TRY(hipMemcpyAsync(result, T.otg.result, (size_t)b->B * sizeof(int), hipMemcpyDeviceToHost, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));
	return SAIP_OK;
}

extern "C" saip_status saip_batch_time_steps(saip_batch* b, int steps, int warmup, double* elapsed_ms) {
	saip_status st = need_ready(b, "saip_batch_time_steps");
	if (st) return st;
	if (steps <= 0 || warmup < 0 || !elapsed_ms) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad timing arguments");
	for (int i = 0; i < warmup; i++)
		if ((st = launch_cycle(b, false))) return st;
	if (!b->time_ev[0]) {
		HIP_TRY(hipEventCreate(&b->time_ev[0]));
		HIP_TRY(hipEventCreate(&b->time_ev[1]));
	}
	hipEvent_t e0 = b->time_ev[0], e1 = b->time_ev[1];
	HIP_TRY(hipEventRecord(e0, b->stream));
	for (int i = 0; i < steps; i++)
		if ((st = launch_cycle(b, false))) return st;
	HIP_TRY(hipEventRecord(e1, b->stream));
	// one wait for the stream (not for the event and then, in the caller, for the stream or the device: each is its own ~15 us
	// marker round trip, tools/bench_overhead_probe.py)
	HIP_TRY(hipStreamSynchronize(b->stream));
	float ms = 0;
	HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
	*elapsed_ms = ms;
	return SAIP_OK;
}

extern "C" saip_status saip_batch_time_steps_begin(saip_batch* b, int steps) {
	saip_status st = need_ready(b, "saip_batch_time_steps_begin");
	if (st) return st;
	if (steps <= 0) return fail(SAIP_ERR_INVALID_ARGUMENT, "bad timing arguments");
	if (!b->time_ev[0]) {
		HIP_TRY(hipEventCreate(&b->time_ev[0]));
		HIP_TRY(hipEventCreate(&b->time_ev[1]));
	}
	HIP_TRY(hipEventRecord(b->time_ev[0], b->stream));
	for (int i = 0; i < steps; i++)
		if ((st = launch_cycle(b, false))) return st;
	HIP_TRY(hipEventRecord(b->time_ev[1], b->stream));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_time_steps_end(saip_batch* b, double* elapsed_ms) {
	saip_status st = need_ready(b, "saip_batch_time_steps_end");
	if (st) return st;
	if (!elapsed_ms || !b->time_ev[0]) return fail(SAIP_ERR_ORDER, "saip_batch_time_steps_end: call saip_batch_time_steps_begin first");
	HIP_TRY(hipEventSynchronize(b->time_ev[1]));  // (returns at once when the caller has waited for the device, as it should have)
	float ms = 0;
	HIP_TRY(hipEventElapsedTime(&ms, b->time_ev[0], b->time_ev[1]));
	*elapsed_ms = ms;
	return SAIP_OK;
}

// ---- robot-model queries (saip_model_query.hip): the batched SaiModel accessors at the resident state
extern "C" saip_status saip_batch_finalize_model_only(saip_batch* b) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "null batch");
	if (b->finalized) return b->model_only ? SAIP_OK : fail(SAIP_ERR_ORDER, "saip_batch_finalize_model_only: the batch is already finalized as a controller");
	if (!b->tasks.empty()) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_finalize_model_only: the batch has tasks (use saip_batch_finalize)");
	if (has_device(b)) {
		HIP_TRY(hipSetDevice(b->device));
		HIP_TRY(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
		const size_t n = b->model->n, ld = b->ld;
		saip_status st;
		if ((st = dev_alloc(b, &b->q, n * ld)) || (st = dev_alloc(b, &b->dq, n * ld)) || (st = dev_alloc(b, &b->model_dev, 1))) return st;
		HIP_TRY(hipMemcpy(b->model_dev, &b->model->dev, sizeof(ModelDev), hipMemcpyHostToDevice));
	}
	b->finalized = true;
	b->model_only = true;
	return SAIP_OK;
}
extern "C" saip_status saip_batch_set_robot_base(saip_batch* b, const double R[9], const double p[3]) {
	if (!b || !R || !p) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_set_robot_base: null argument");
	for (int i = 0; i < 9; i++)
		if (!std::isfinite(R[i])) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_set_robot_base: non-finite rotation");
	for (int i = 0; i < 3; i++)
		if (!std::isfinite(p[i])) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_set_robot_base: non-finite translation");
	memcpy(b->base_R, R, sizeof(b->base_R));
	memcpy(b->base_p, p, sizeof(b->base_p));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_get_robot_base(const saip_batch* b, double R[9], double p[3]) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "saip_batch_get_robot_base: null batch");
	if (R) memcpy(R, b->base_R, sizeof(b->base_R));
	if (p) memcpy(p, b->base_p, sizeof(b->base_p));
	return SAIP_OK;
}
extern "C" int saip_batch_model_frame_rows(const saip_batch* b, int flags) {
	if (!b || !b->model || (flags & ~(SAIP_QUERY_JACOBIAN | SAIP_QUERY_WORLD))) return 0;
	return 18 + ((flags & SAIP_QUERY_JACOBIAN) ? 6 * b->model->n : 0);
}
// the _host scratch: grown to the largest query seen, never shrunk
static saip_status query_scratch(saip_batch* b, size_t rows) {
	if (rows <= b->query_rows) return SAIP_OK;
	saip_status st = dev_alloc(b, &b->query_dev, rows * b->ld);
	if (st) return st;
	b->query_rows = rows;
	return SAIP_OK;
}
// argument errors come before the device check, so that they show on a configuration-only batch as well
static saip_status check_frames(saip_batch* b, int nf, const int* links, int flags, const double* out, const char* fn) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null batch", fn);
	if (!b->finalized) return fail(SAIP_ERR_ORDER, "%s: call saip_batch_finalize first", fn);
	if (nf < 1 || nf > SAIP_MAX_QUERY_FRAMES) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: n_frames %d outside 1..%d", fn, nf, SAIP_MAX_QUERY_FRAMES);
	if (!links || !out) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null links or output", fn);
	if (flags & ~(SAIP_QUERY_JACOBIAN | SAIP_QUERY_WORLD)) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: unknown flag bits 0x%x", fn, flags);
	const int nl = (int)b->model->links.size();
	for (int f = 0; f < nf; f++)
		if (links[f] < 0 || links[f] >= nl) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: link index %d out of range (%d links)", fn, links[f], nl);
	return need_state(b, fn);
}
static saip_status launch_frames(saip_batch* b, int nf, const int* links, const double* pos_in_link, int flags, double* out_dev, const char* fn) {
	saip_status st = check_frames(b, nf, links, flags, out_dev, fn);
	if (st) return st;
	saip::FrameQuery Q;
	memset(&Q, 0, sizeof(Q));
	Q.B = b->B;
	Q.ld = b->ld;
	Q.n = b->model->n;
	Q.nf = nf;
	Q.rows = saip_batch_model_frame_rows(b, flags);
	Q.jac = (flags & SAIP_QUERY_JACOBIAN) ? 1 : 0;
	Q.world = (flags & SAIP_QUERY_WORLD) ? 1 : 0;
	// frames sorted by body (stable: one walk emits them in order); the constants are composed exactly as saip_batch_add_motion_force_task
	// composes a task's control frame, so that a frame equal to one is bit-identical to the pose readback
	int order[SAIP_MAX_QUERY_FRAMES];
	for (int f = 0; f < nf; f++) order[f] = f;
	for (int i = 1; i < nf; i++)
		for (int k = i; k > 0 && b->model->links[links[order[k - 1]]].body > b->model->links[links[order[k]]].body; k--) std::swap(order[k - 1], order[k]);
	double I3[9];
	m3_eye(I3);
	for (int i = 0; i < nf; i++) {
		const int f = order[i];
		const LinkInfo& L = b->model->links[links[f]];
		const double zero[3] = {0, 0, 0};
		double t[3];
		m3_vec(L.R, pos_in_link ? pos_in_link + 3 * f : zero, t);
		for (int e = 0; e < 3; e++) Q.pos[i][e] = L.p[e] + t[e];
		m3_mul(L.R, I3, Q.rot[i]);
		Q.body[i] = L.body;
		Q.slot[i] = f;
	}
	memcpy(Q.Rwb, b->base_R, sizeof(Q.Rwb));
	memcpy(Q.pwb, b->base_p, sizeof(Q.pwb));
	Q.model = b->model_dev;
	Q.q = b->q;
	Q.dq = b->dq;
	Q.out = out_dev;
	hipError_t e = saip::launch_model_frames(Q, b->model->dev.is_tree != 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "model frames kernel launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_model_frames_device(saip_batch* b, int n_frames, const int* links, const double* pos_in_link, int flags, double* out_dev) {
	return launch_frames(b, n_frames, links, pos_in_link, flags, out_dev, "saip_batch_model_frames_device");
}
extern "C" saip_status saip_batch_model_frames_host(saip_batch* b, int n_frames, const int* links, const double* pos_in_link, int flags, double* out) {
	const char* fn = "saip_batch_model_frames_host";
	saip_status st = check_frames(b, n_frames, links, flags, out, fn);
	if (st) return st;
	const int rows = saip_batch_model_frame_rows(b, flags);
	if ((st = query_scratch(b, (size_t)n_frames * rows))) return st;
	if ((st = launch_frames(b, n_frames, links, pos_in_link, flags, b->query_dev, fn))) return st;
	HIP_TRY(hipStreamSynchronize(b->stream));
	return copy_d2h(b, out, b->query_dev, n_frames * rows);
}
static saip_status check_dynamics(saip_batch* b, bool any_output, const char* fn) {
	if (!b) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: null batch", fn);
	if (!b->finalized) return fail(SAIP_ERR_ORDER, "%s: call saip_batch_finalize first", fn);
	if (!any_output) return fail(SAIP_ERR_INVALID_ARGUMENT, "%s: every output is NULL", fn);
	return need_state(b, fn);
}
static saip_status launch_dynamics(saip_batch* b, double* M, double* Minv, double* g, double* h, const char* fn) {
	saip_status st = check_dynamics(b, M || Minv || g || h, fn);
	if (st) return st;
	saip::DynQuery Q;
	memset(&Q, 0, sizeof(Q));
	Q.B = b->B;
	Q.ld = b->ld;
	Q.n = b->model->n;
	Q.model = b->model_dev;
	Q.q = b->q;
	Q.dq = b->dq;
	Q.M = M;
	Q.Minv = Minv;
	Q.g = g;
	Q.h = h;
	hipError_t e = saip::launch_model_dynamics(Q, b->model->dev.is_tree != 0, b->stream);
	if (e != hipSuccess) return fail(SAIP_ERR_DEVICE, "model dynamics kernel launch failed: %s", hipGetErrorString(e));
	return SAIP_OK;
}
extern "C" saip_status saip_batch_model_dynamics_device(saip_batch* b, double* M_dev, double* M_inv_dev, double* g_dev, double* b_dev) {
	return launch_dynamics(b, M_dev, M_inv_dev, g_dev, b_dev, "saip_batch_model_dynamics_device");
}
extern "C" saip_status saip_batch_model_dynamics_host(saip_batch* b, double* M, double* M_inv, double* g, double* bias) {
	const char* fn = "saip_batch_model_dynamics_host";
	saip_status st = check_dynamics(b, M || M_inv || g || bias, fn);
	if (st) return st;
	const size_t n = b->model->n, ld = b->ld;
	if ((st = query_scratch(b, 2 * n * n + 2 * n))) return st;  // M, M^-1, g, b blocks
	double* d = b->query_dev;
	if ((st = launch_dynamics(b, M ? d : nullptr, M_inv ? d + n * n * ld : nullptr, g ? d + 2 * n * n * ld : nullptr, bias ? d + (2 * n * n + n) * ld : nullptr, fn)))
		return st;
	HIP_TRY(hipStreamSynchronize(b->stream));
	if (M && (st = copy_d2h(b, M, d, (int)(n * n)))) return st;
	if (M_inv && (st = copy_d2h(b, M_inv, d + n * n * ld, (int)(n * n)))) return st;
	if (g && (st = copy_d2h(b, g, d + 2 * n * n * ld, (int)n))) return st;
	if (bias && (st = copy_d2h(b, bias, d + (2 * n * n + n) * ld, (int)n))) return st;
	return SAIP_OK;
}

extern "C" const char* saip_last_error(void) { return g_err.c_str(); }
extern "C" const char* saip_version(void) { return "saip 0.1 (gfx950)"; }
