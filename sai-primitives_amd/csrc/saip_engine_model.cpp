// The URDF-style model builder behind saip_model_*: links merged into movable bodies, the constants the kernels read (ModelDev),
// and the small 3x3 helpers the other units compose frames with.
#include "saip_engine_internal.h"

// ------------------------------------------------------------------ tiny 3x3 helpers (row-major)
void saip::eng::m3_mul(const double* A, const double* B, double* C) {
	double T[9];
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < 3; j++) T[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
	memcpy(C, T, sizeof(T));
}
void saip::eng::m3_vec(const double* A, const double* v, double* o) {
	double t[3];
	for (int i = 0; i < 3; i++) t[i] = A[3 * i] * v[0] + A[3 * i + 1] * v[1] + A[3 * i + 2] * v[2];
	memcpy(o, t, sizeof(t));
}
void saip::eng::m3_T(const double* A, double* B) {
	double T[9];
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < 3; j++) T[3 * i + j] = A[3 * j + i];
	memcpy(B, T, sizeof(T));
}
void saip::eng::m3_eye(double* A) {
	memset(A, 0, 9 * sizeof(double));
	A[0] = A[4] = A[8] = 1.0;
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
int saip::eng::range_basis_3(const double* dirs, int cnt, double* basis) {
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
