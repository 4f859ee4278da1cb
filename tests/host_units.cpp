// host_units.cpp -- stand-alone driver of lq_mpc_amd/csrc/lqmpc_host.h for tests/test_host_units_cpu.py (built with the address and
// undefined-behaviour sanitizers).  Reads cases from the file named on the command line, prints one result line per case.
//   arena n  (bytes out present) x n     -> "arena in_end total off_0 .. off_{n-1}", after writing every byte of every array into a
//                                           heap block of exactly `total` bytes
//   inv n  M (n x n)                     -> "inv ok M^-1"
//   eig n  M (n x n)                     -> "eig ok emax emin"
//   gain nx nu N  A B Q R P              -> "gain ok K (nu x nx)"
#include "../lq_mpc_amd/csrc/lqmpc_host.h"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>

static std::vector<double> read(std::istream &f, int count)
{
    std::vector<double> v(count);
    for (double &x : v) f >> x;
    return v;
}

static void show(const std::vector<double> &v)
{
    for (double x : v) printf(" %.17g", x);
    printf("\n");
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    std::ifstream f(argv[1]);
    std::string what;
    while (f >> what) {
        if (what == "arena") {
            int n;
            f >> n;
            lqmpc::ArenaLayout lay;
            for (int k = 0; k < n; ++k) {
                size_t bytes;
                int out, present;
                f >> bytes >> out >> present;
                lay.add(bytes, out != 0, present != 0);
            }
            lay.place();
            char *block = new char[lay.total];
            for (const auto &s : lay.slots)
                if (s.present) memset(block + s.off, 0x5a, s.bytes);
            delete[] block;
            printf("arena %zu %zu", lay.in_end, lay.total);
            for (const auto &s : lay.slots) printf(" %zu", s.off);
            printf("\n");
        } else if (what == "inv") {
            int n;
            f >> n;
            std::vector<double> M = read(f, n * n);
            const bool ok = host_spd_inverse(M, n);
            printf("inv %d", ok ? 1 : 0);
            show(M);
        } else if (what == "eig") {
            int n;
            f >> n;
            const std::vector<double> M = read(f, n * n);
            double emax = 0.0, emin = 0.0;
            const bool ok = host_sym_eig_extremes(M.data(), n, emax, emin);
            printf("eig %d", ok ? 1 : 0);
            show({emax, emin});
        } else if (what == "gain") {
            int nx, nu, N;
            f >> nx >> nu >> N;
            const std::vector<double> A = read(f, nx * nx), B = read(f, nx * nu), Q = read(f, nx * nx), R = read(f, nu * nu), P = read(f, nx * nx);
            std::vector<double> K(nu * nx, 0.0);
            const bool ok = host_first_gain(nx, nu, N, A.data(), B.data(), Q.data(), R.data(), P.data(), K.data());
            printf("gain %d", ok ? 1 : 0);
            show(K);
        } else {
            return 3;
        }
    }
    return f.eof() ? 0 : 4;
}
