"""The fp32 front end's noise floor on the edge inputs of tests/golden/ref_e2e.npz (diagnostic, CPU only): the chain with the window, the
pre-emphasis, the mean removal and the transform in IEEE float32 - a packed real FFT as the kernels run it, once with bigfft_kernel's radix-2
Stockham passes and once with a correctly rounded half-size complex transform - and everything behind the power spectrum in float64, against
the rows the compiled reference wrote.  Prints worst element-wise error / worst error against the row's largest value."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
from oracle.oracle import Oracle
from tests.util import *
fx=ref_e2e()
f32=np.float32
def stockham_packed(buf):
    """bigfft_kernel's transform in IEEE float32: packed real FFT, Stockham radix-2, table twiddles rounded from double, untangle."""
    N=buf.size; Nc=N//2
    tw=np.exp(-2j*np.pi*np.arange(Nc)/N).astype(np.complex64)
    src=(buf[0::2].astype(f32)+1j*buf[1::2].astype(f32)).astype(np.complex64)
    Ns=1
    while Ns<Nc:
        tstep=Nc//Ns; j=np.arange(Nc//2); k=j&(Ns-1)
        w=tw[k*tstep]; a=src[j]; b0=src[j+Nc//2]
        b=((b0.real*w.real-b0.imag*w.imag).astype(f32)+1j*(b0.real*w.imag+b0.imag*w.real).astype(f32)).astype(np.complex64)
        dst=np.zeros(Nc,np.complex64); j0=((j-k)<<1)+k
        dst[j0]=a+b; dst[j0+Ns]=a-b
        src=dst; Ns<<=1
    P=np.zeros(Nc+1,f32)
    k=np.arange(1,Nc); a=src[k]; c=src[Nc-k]; w=tw[k]
    sr=a.real+c.real; si=a.imag-c.imag; dr=a.real-c.real; di=a.imag+c.imag
    tr=(w.real*di+w.imag*dr).astype(f32); ti=(w.imag*di-w.real*dr).astype(f32)
    ur=sr+tr; ui=si+ti
    P[1:Nc]=f32(0.25)*(ur*ur+ui*ui)
    v=src[0].real-src[0].imag; P[Nc]=v*v
    return P.astype(np.float64)
def pocket_packed(buf):
    """a packed real FFT with an accurate complex64 half-size transform and the untangle in float32"""
    N=buf.size; Nc=N//2
    tw=np.exp(-2j*np.pi*np.arange(Nc)/N).astype(np.complex64)
    z=(buf[0::2].astype(f32)+1j*buf[1::2].astype(f32)).astype(np.complex64)
    src=np.fft.fft(z); assert src.dtype==np.complex64
    P=np.zeros(Nc+1,f32)
    k=np.arange(1,Nc); a=src[k]; c=src[Nc-k]; w=tw[k]
    sr=a.real+c.real; si=a.imag-c.imag; dr=a.real-c.real; di=a.imag+c.imag
    tr=(w.real*di+w.imag*dr).astype(f32); ti=(w.imag*di-w.real*dr).astype(f32)
    ur=sr+tr; ui=si+ti
    P[1:Nc]=f32(0.25)*(ur*ur+ui*ui)
    v=src[0].real-src[0].imag; P[Nc]=v*v
    return P.astype(np.float64)
def chain(cfg,u,fft):
    o=Oracle(cfg); d=o.dims; W,S,N,B=d.window,d.wshift,d.wfft,d.B
    ham=o.hamming().astype(f32); pre=f32(o.preem()); mat,_,_=o.fbank()
    T=(u.size-W)//S+1; x=u.astype(f32); rows=[]; nc=d.D-1
    i=np.arange(1,nc+1)[:,None]; k=np.arange(B)[None,:]
    dct=np.sqrt(2.0/B)*np.cos(np.pi*i*(k+0.5)/B); lift=1+11*np.sin(np.pi*np.arange(1,nc+1)/22)
    for t in range(T):
        s=t*S; fr=x[s:s+W]; prev=np.concatenate([[x[s-1] if s>0 else f32(0)],fr[:-1]]).astype(f32)
        y=(ham*(fr-pre*prev)).astype(f32); y=(y-f32(y.astype(np.float64).sum()/W)).astype(f32)   # float32 front end
        buf=np.zeros(N,f32); buf[:W]=y
        P=fft(buf); P[0]=1e-10
        L=np.log(mat@P); c=dct@L*lift
        rows.append(np.concatenate([c,[np.sqrt(2.0/B)*L.sum()]]))
    return np.array(rows)
def errs(g,ref):
    dd=np.abs(g-ref); return "%.3e / %.3e"%(float((dd/np.maximum(np.abs(ref),1)).max()), float((dd.max(1)/np.maximum(np.abs(ref).max(1),1)).max()))
for case,gen in (("edge_f","sine_fs_4"),("edge_g","alt_fs"),("edge_a","alt_fs"),("edge_f","alt_fs"),("edge_f","clipped")):
    cfg,inp=REF_E2E_CASES[case]; i=EDGE_INPUTS.index(gen); u=ref_e2e_inputs(inp)[i]
    ref=fx[f"{case}__{i}__rows"].astype(np.float64)
    print(case,gen,"stockham radix-2 f32:",errs(chain(cfg,u,stockham_packed),ref)," accurate c64 + f32 untangle:",errs(chain(cfg,u,pocket_packed),ref))
