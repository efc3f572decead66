"""Writes tests/golden/turtlebot3_world_ndt.npz: the NDT map of beluga_example (maps/turtlebot3_world.hdf5) as the four datasets
io::load_from_hdf5 reads (ndt_sensor_model.hpp): cells[n,2] int32, means[n,2], covariances[n,2,2], resolution.

Run once, by hand, where the reference checkout and an HDF5 1.10 shared library are at hand (there is no h5py: the C library is
called through ctypes):

    python tests/golden/make_turtlebot_ndt.py /path/to/turtlebot3_world.hdf5 /path/to/libhdf5.so
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def read_hdf5(path, lib_path):
    h5 = C.CDLL(lib_path)
    hid_t = C.c_int64
    h5.H5open()
    h5.H5Fopen.restype = hid_t
    h5.H5Fopen.argtypes = [C.c_char_p, C.c_uint, hid_t]
    h5.H5Dopen2.restype = hid_t
    h5.H5Dopen2.argtypes = [hid_t, C.c_char_p, hid_t]
    h5.H5Dget_space.restype = hid_t
    h5.H5Dget_space.argtypes = [hid_t]
    h5.H5Sget_simple_extent_ndims.argtypes = [hid_t]
    h5.H5Sget_simple_extent_dims.argtypes = [hid_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    h5.H5Dread.argtypes = [hid_t, hid_t, hid_t, hid_t, hid_t, C.c_void_p]
    h5.H5Dclose.argtypes = [hid_t]
    h5.H5Sclose.argtypes = [hid_t]
    h5.H5Fclose.argtypes = [hid_t]
    native_double = hid_t.in_dll(h5, "H5T_NATIVE_DOUBLE_g").value
    native_int = hid_t.in_dll(h5, "H5T_NATIVE_INT_g").value
    f = h5.H5Fopen(path.encode(), 0, 0)  # H5F_ACC_RDONLY, H5P_DEFAULT
    if f < 0:
        raise RuntimeError(f"cannot open {path}")

    def dataset(name, dtype, h5type):
        d = h5.H5Dopen2(f, name.encode(), 0)
        if d < 0:
            raise RuntimeError(f"no dataset {name}")
        space = h5.H5Dget_space(d)
        ndims = h5.H5Sget_simple_extent_ndims(space)
        dims = (C.c_uint64 * max(ndims, 1))()
        h5.H5Sget_simple_extent_dims(space, dims, None)
        shape = tuple(dims[k] for k in range(ndims))
        out = np.zeros(shape, dtype=dtype)
        if h5.H5Dread(d, h5type, 0, 0, 0, out.ctypes.data) < 0:  # H5S_ALL, H5S_ALL, H5P_DEFAULT
            raise RuntimeError(f"cannot read {name}")
        h5.H5Sclose(space)
        h5.H5Dclose(d)
        return out

    z = dict(means=dataset("means", np.float64, native_double), covariances=dataset("covariances", np.float64, native_double),
             cells=dataset("cells", np.int32, native_int), resolution=dataset("resolution", np.float64, native_double))
    h5.H5Fclose(f)
    return z


def main():
    src, lib = sys.argv[1], sys.argv[2]
    z = read_hdf5(src, lib)
    n = len(z["cells"])
    np.savez_compressed(os.path.join(HERE, "turtlebot3_world_ndt.npz"), cells=z["cells"].reshape(n, 2).astype(np.int32),
                        means=z["means"].reshape(n, 2), covariances=z["covariances"].reshape(n, 2, 2),
                        resolution=np.float64(z["resolution"].reshape(-1)[0]))
    print(f"{n} cells, resolution {float(z['resolution'].reshape(-1)[0])}")


if __name__ == "__main__":
    main()
